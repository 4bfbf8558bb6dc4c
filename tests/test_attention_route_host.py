"""Host side of the attention launches (no GPU): the rows the four uniform forms of the AR steps name (tests/attn_ref.py against
rows written out by hand), the uniform and the ragged statement of the same launch, and attn_route (csrc/attention.hip, through
mt2_attention_route) on the shapes the model launches, on every rejection and on a restatement of the whole ladder."""
import ctypes
import math
import os
import re

import numpy as np
import pytest

import attn_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID = 1          # hipErrorInvalidValue


@pytest.fixture(scope="module")
def rt():
    from megatts2_amd import runtime
    return runtime


# ---- the four model forms ------------------------------------------------------------------------------------------------------

A, N, H, D = 3, 5, 2, 32
# form -> per sequence (first query row, queries, first key row, keys, first output row), counted from the pointers passed, and the
# BUFFER row the Q pointer is at
FORM_ROWS = {
    "full": ([(0, 5, 0, 5, 0), (5, 5, 5, 5, 5), (10, 5, 10, 5, 10)], 3),
    "last-compact": ([(0, 1, 0, 5, 0), (1, 1, 5, 5, 1), (2, 1, 10, 5, 2)], 3),
    "last-fused": ([(0, 1, 0, 5, 0), (5, 1, 5, 5, 1), (10, 1, 10, 5, 2)], 3 + 4),        # the Q pointer sits n - 1 rows further
    "cached": ([(0, 5, 0, 5, 0), (12, 5, 12, 5, 5), (24, 5, 24, 5, 10)], 3),            # slots of cs = n + 7 rows, compact output
}


@pytest.mark.parametrize("name", R.FORMS)
def test_model_forms_name_the_rows_of_the_table(name):
    f = R.model_form(name, A, N, H, D)
    want, qrow = FORM_ROWS[name]
    assert R.ranges(f.g) == want
    assert f.q[1] == qrow and f.k[1] == 3 and f.v[1] == 3 and f.o[1] == 3
    d = H * D
    if name == "last-compact":
        assert (f.ldq, f.ldk, f.ldv, f.ldo) == (d, 2 * d, 2 * d, d) and (f.q[2], f.k[2], f.v[2]) == (0, 0, d)
        assert f.g.max_qlen == 1 and f.g.u_ostride == 0
    else:
        assert (f.ldq, f.ldk, f.ldv, f.ldo) == (3 * d, 3 * d, 3 * d, d) and (f.q[2], f.k[2], f.v[2]) == (0, d, 2 * d)
    # the query rows in the buffer: the last row of every sequence for both last-row forms
    qbuf = [f.q[1] + qs + i for qs, ql, _, _, _ in want for i in range(ql)]
    assert qbuf == f.live["q"]
    if name == "last-fused":
        assert qbuf == [3 + b * N + N - 1 for b in range(A)] and f.g.u_ostride == 1 and f.g.u_qstride == N
    if name == "cached":
        assert f.g.u_ostride == N and f.g.u_qstride == N + 7 == f.g.u_kvstride
    # what the launch may read is finite, everything else of Q / K / V is not
    bufs = R.fill(f, np.random.default_rng(1), spike_seq=1)
    for op, at in (("q", f.q), ("k", f.k), ("v", f.v)):
        cols = bufs[at[0]][:, at[2]:at[2] + d]
        live = np.zeros(cols.shape[0], bool)
        live[f.live[op]] = True
        assert np.isfinite(cols[live]).all() and np.isnan(cols[~live]).all()
        assert not live[:R.LEAD].any() and not live[-R.TRAIL:].any()


def softmax_rows(q, k, v, scale):
    s = q.astype(np.float64) @ k.astype(np.float64).T * scale
    p = np.exp(s - s.max(1, keepdims=True))
    return (p / p.sum(1, keepdims=True)) @ v.astype(np.float64)


@pytest.mark.parametrize("name", R.FORMS)
def test_reference_of_a_uniform_launch(name):
    """attention_ref on a uniform form: against attention written out on the BUFFER rows by hand, against the ragged launch that
    names the same rows, and its write set."""
    f = R.model_form(name, A, N, H, D)
    d, scale = H * D, 1.0 / math.sqrt(D)
    bufs = R.fill(f, np.random.default_rng(2), spike_seq=2)
    Q, K, V = (R.view(bufs, at) for at in (f.q, f.k, f.v))
    O, rows = R.attention_ref(Q, K, V, f.g, scale, f.o_rows)
    last = name.startswith("last")
    stride = N + 7 if name == "cached" else N
    qkv = bufs["kv"] if name == "last-compact" else bufs["qkv"]
    kcol, vcol = (0, d) if name == "last-compact" else (d, 2 * d)
    for b in range(A):
        first = 3 + b * stride
        if name == "last-compact":
            q = bufs["q"][3 + b:4 + b]
        elif name == "last-fused":
            q = qkv[first + N - 1:first + N, :d]
        else:
            q = qkv[first:first + N, :d]
        for h in range(H):
            sl = slice(h * D, (h + 1) * D)
            want = softmax_rows(q[:, sl], qkv[first:first + N, kcol:kcol + d][:, sl], qkv[first:first + N, vcol:vcol + d][:, sl], scale)
            o0 = b if last else b * N
            assert np.allclose(O[o0:o0 + q.shape[0], sl], want, rtol=1e-13, atol=1e-15)
    assert rows.tolist() == (list(range(A)) if last else list(range(A * N)))
    assert not O[rows[-1] + 1:].any()
    gr = R.as_ragged(f.g)
    assert gr.ragged and gr.max_kvlen == N and R.ranges(gr) == R.ranges(f.g)
    Or, rows_r = R.attention_ref(Q, K, V, gr, scale, f.o_rows)
    assert np.array_equal(O, Or) and np.array_equal(rows, rows_r)
    # one sequence launched alone names the same rows once the pointers have moved
    for b in range(A):
        g1, (dq, dk, do) = R.one_sequence(f.g, b)
        O1, rows1 = R.attention_ref(Q[dq:], K[dk:], V[dk:], g1, scale, f.o_rows - do)
        assert np.array_equal(O1[rows1], O[rows1 + do]) and np.array_equal(rows1 + do, rows[rows1.size * b:rows1.size * (b + 1)])


def test_reference_of_a_ragged_launch_with_output_rows_of_its_own():
    """o_start moves the output rows and nothing else; an empty key range writes nothing."""
    rng = np.random.default_rng(3)
    Q, K, V = (rng.standard_normal((40, H * D)).astype(np.float32) for _ in range(3))
    i32 = lambda *x: np.asarray(x, np.int32)
    g = R.Geometry(B=3, H=H, D=D, max_qlen=7, q_start=i32(2, 20, 9), q_len=i32(7, 3, 4), kv_start=i32(0, 30, 11), kv_len=i32(9, 0, 6))
    O, rows = R.attention_ref(Q, K, V, g, 0.25, 40)
    assert rows.tolist() == list(range(2, 9)) + list(range(9, 13))
    from dataclasses import replace
    O2, rows2 = R.attention_ref(Q, K, V, replace(g, o_start=i32(30, 0, 1)), 0.25, 40)
    assert rows2.tolist() == list(range(1, 5)) + list(range(30, 37))
    assert np.array_equal(O2[30:37], O[2:9]) and np.array_equal(O2[1:5], O[9:13])
    assert np.allclose(O[9:13, D:], softmax_rows(Q[9:13, D:], K[11:17, D:], V[11:17, D:], 0.25), rtol=1e-13, atol=1e-15)
    # the float32 restatement, on the per-row measure the GPU test uses: well inside the bar of 3e-6
    worst = max(e[3] for e in R.block_errors(R.attention_f32(Q, K, V, g, 0.25, 40), O, g))
    assert 0 < worst < 1e-6


# ---- the route -----------------------------------------------------------------------------------------------------------------

DEFAULTS = dict(lds_min_qlen=640, x6_min_qlen=192, lds_waves=0, ds_short=1, x3h=0, o_planes=0)      # AttnP's and EngineOpts' defaults


def route(rt, D, n, H=2, B=3, *, max_qlen=None, ragged=False, max_kvlen=0, ld=None, **over):
    """The route of a self-attention launch over B sequences of n positions (uniform, or ragged with the arrays present)."""
    d = H * D
    ld = dict(dict(ldq=3 * d, ldk=3 * d, ldv=3 * d, ldo=d), **(ld or {}))
    opts = dict(DEFAULTS, **over)
    geo = dict(q_start=64, q_len=64, kv_start=64, kv_len=64, max_kvlen=max_kvlen) if ragged else \
        dict(u_qstride=n, u_qlen=n if max_qlen is None else max_qlen, u_kvstride=n, u_kvlen=n)
    O = opts.pop("O", 128)
    return rt.attention_route(ld["ldq"], ld["ldk"], ld["ldv"], ld["ldo"], O=O, B=B, H=H, D=D, max_qlen=n if max_qlen is None else max_qlen,
                              scale=1.0, **geo, **opts)


@pytest.mark.parametrize("D", [64, 96])
def test_route_of_the_ar_steps(rt, D):
    NS = D // 32
    for n, nkv in ((1, 1), (32, 1), (33, 2), (128, 4)):
        r = route(rt, D, n)
        assert (r["err"], r["kernel"], r["d"], r["nkv"]) == (0, "ds", D, nkv), (n, r)
        assert r["grid"] == ((n + 31) // 32, 2, 3) and r["block"] == 64 * nkv * NS and r["lds"] == nkv * NS * 34 * 64 * 4
    r = route(rt, D, 129)
    assert (r["err"], r["kernel"], r["d"], r["nwv"]) == (0, "reg", D, 4), r
    assert r["grid"] == (5, 2, 3) and r["block"] == 256 and r["lds"] == 3 * (NS * 16 + 2) * 64 * 4
    assert route(rt, D, 128, ds_short=0)["kernel"] == "reg"
    r = route(rt, D, 40, ds_short=0)
    assert (r["kernel"], r["nwv"], r["block"], r["lds"]) == ("reg", 2, 128, (NS * 16 + 2) * 64 * 4)
    assert route(rt, D, 20, ds_short=0)["lds"] == 0                 # one wave: nothing to merge
    # the last layer: one query per sequence, however long the history
    r = route(rt, D, 500, max_qlen=1)
    assert (r["kernel"], r["nwv"], r["grid"]) == ("reg", 4, (1, 2, 3)), r
    assert route(rt, D, 100, max_qlen=1)["kernel"] == "ds"
    # the matrix-pipe kernel from x6_min_qlen queries on, the LDS-tiled kernel behind it
    assert route(rt, D, 191)["kernel"] == "reg"
    r = route(rt, D, 192)
    assert (r["kernel"], r["d"], r["nwq"], r["grid"], r["block"]) == ("x6", D, 4, (2, 2, 3), 256), r
    assert r["lds"] == 3 * (32 * (2 * D + 16) + 80 * D)
    r = route(rt, D, 192, x3h=1)
    assert (r["kernel"], r["nwq"], r["lds"]) == ("x3h", 4, 2 * (32 * (2 * D + 16) + 80 * D)), r
    for n, waves, nwq in ((599, 0, 4), (600, 0, 8), (700, 4, 4), (200, 8, 8)):       # as launch_attn_x6_d decided
        for x3h in (0, 1):
            r = route(rt, D, n, lds_waves=waves, x3h=x3h)
            assert (r["kernel"], r["nwq"], r["block"]) == ("x3h" if x3h else "x6", nwq, 64 * nwq), (n, waves, r)
            assert r["grid"][0] == -(-n // (32 * nwq))
    assert route(rt, D, 639, x6_min_qlen=0)["kernel"] == "reg"
    r = route(rt, D, 640, x6_min_qlen=0)
    assert (r["kernel"], r["d"], r["nwq"], r["lds"], r["grid"][0]) == ("lds", D, 4, 4 * 32 * (D + 4) * 4, 5), r
    assert route(rt, D, 640, x6_min_qlen=0, lds_waves=8)["nwq"] == 8
    assert route(rt, D, 640, x6_min_qlen=0, lds_min_qlen=0)["kernel"] == "reg"
    assert route(rt, D, 640, x6_min_qlen=0, ld=dict(ldv=3 * 2 * D + 2))["kernel"] == "reg"       # the LDS loader reads V as float4


@pytest.mark.parametrize("D", [32, 128])
def test_route_never_splits_the_head_dim_or_leaves_f32_at_32_and_128(rt, D):
    for n in (1, 33, 128, 129, 192, 300, 639, 640, 900):
        for over in ({}, dict(x6_min_qlen=1), dict(x3h=1, x6_min_qlen=1), dict(ds_short=1, max_qlen=1)):
            r = route(rt, D, n, **over)
            want = "lds" if (n >= 640 and over.get("max_qlen") is None) else "reg"
            assert (r["err"], r["kernel"], r["d"]) == (0, want, D), (n, over, r)


def test_route_of_the_wide_heads(rt):
    for D, dt, nw in ((256, 4, 2), (512, 4, 4), (160 + 32, 3, 2), (384, 4, 3)):
        for n in (40, 700):
            r = route(rt, D, n, x6_min_qlen=1, lds_min_qlen=1)
            assert (r["err"], r["kernel"], r["d"], r["nwv"], r["block"], r["lds"]) == (0, "generic", dt, nw, 64 * nw, 0), (D, r)
            assert r["grid"] == ((n + 31) // 32, 2, 3)


def test_route_of_ragged_launches(rt):
    for D in (64, 96):
        r = route(rt, D, 50, ragged=True, max_kvlen=0)
        assert (r["kernel"], r["nwv"]) == ("reg", 2), r           # no key bound: as long as the queries, and never the ds kernel
        assert route(rt, D, 1, ragged=True, max_kvlen=0)["kernel"] == "reg"
        r = route(rt, D, 50, ragged=True, max_kvlen=128)
        assert (r["kernel"], r["nkv"]) == ("ds", 4), r
        assert route(rt, D, 50, ragged=True, max_kvlen=129)["kernel"] == "reg"
        assert route(rt, D, 50, ragged=True, max_kvlen=700)["nwv"] == 4
        assert route(rt, D, 200, ragged=True, max_kvlen=10)["kernel"] == "x6"


def test_route_rejections_stand_beside_the_launch_they_differ_from(rt):
    ok = lambda r: r["err"] == 0 and r["kernel"] != "none"
    bad = lambda r: r["err"] == INVALID and r["kernel"] == "none"
    assert ok(route(rt, 64, 40)) and bad(route(rt, 48, 40)) and bad(route(rt, 80, 40))
    d = 128
    for name, good in (("ldq", 3 * d), ("ldk", 3 * d), ("ldo", d)):
        assert ok(route(rt, 64, 40, ld={name: good + 4})), name
        for off in (1, 2, 3):
            assert bad(route(rt, 64, 40, ld={name: good + off})), (name, off)
    assert ok(route(rt, 64, 40, ld=dict(ldv=3 * d + 1)))                      # V is read by element everywhere but in the LDS loader
    # fp16 planes: whole 128-byte blocks per output row
    assert ok(route(rt, 64, 40, o_planes=1)) and ok(route(rt, 64, 40, o_planes=1, ld=dict(ldo=d + 32)))
    assert bad(route(rt, 64, 40, o_planes=1, ld=dict(ldo=d + 16))) and ok(route(rt, 64, 40, o_planes=0, ld=dict(ldo=d + 16)))
    assert bad(route(rt, 64, 40, o_planes=1, O=128 + 64)) and ok(route(rt, 64, 40, o_planes=0, O=128 + 64))
    assert ok(route(rt, 64, 40, o_planes=1, O=256))
    # wide heads: <= 4 waves of <= 4 tiles each, the tiles dealt evenly
    for D, fine in ((192, True), (160, False), (224, False), (256, True), (512, True), (544, False), (640, False), (1024, False)):
        r = route(rt, D, 40)
        assert ok(r) if fine else bad(r), (D, r)


def test_route_with_nothing_to_launch(rt):
    for over in (dict(B=0), dict(B=-1), dict(H=0), dict(max_qlen=0), dict(max_qlen=-3)):
        r = route(rt, 64, 40, **over)
        assert (r["err"], r["kernel"]) == (0, "none"), over
    assert route(rt, 48, 40, B=0)["err"] == 0           # ... before anything is looked at


def restated(D, max_qlen, kvmax_uniform, ragged, max_kvlen, ldv, o):
    """The ladder of attn_route written from the comments of csrc/mt2_kernels.h (AttnP) for launches that are not rejected."""
    if D in (64, 96) and o["x6_min_qlen"] > 0 and max_qlen >= o["x6_min_qlen"]:
        nwq = 8 if o["lds_waves"] == 8 or (o["lds_waves"] != 4 and max_qlen >= 600) else 4
        return ("x3h" if o["x3h"] else "x6", nwq)
    if D <= 128 and o["lds_min_qlen"] > 0 and max_qlen >= o["lds_min_qlen"] and ldv % 4 == 0:
        return ("lds", 8 if o["lds_waves"] == 8 else 4)
    if D <= 128:
        bound = (max_kvlen if max_kvlen > 0 else max_qlen) if ragged else kvmax_uniform
        known = (not ragged) or max_kvlen > 0
        tiles = max(1, -(-bound // 32))
        if o["ds_short"] and D in (64, 96) and bound <= 128 and known:
            return ("ds", tiles)
        return ("reg", min(4, tiles))
    nw = -(-D // 128)
    while (D // 32) % nw:
        nw += 1
    return ("generic", nw)


def test_route_agrees_with_its_restatement_on_a_grid(rt):
    seen = set()
    for D in (32, 64, 96, 128, 256, 512):
        for n in (1, 32, 33, 128, 129, 191, 192, 599, 600, 639, 640, 834):
            for max_qlen in (1, n):
                for ragged, max_kvlen in ((False, 0), (True, 0), (True, n)):
                    for o in (DEFAULTS, dict(DEFAULTS, x6_min_qlen=0), dict(DEFAULTS, x6_min_qlen=1, x3h=1, lds_waves=8),
                              dict(DEFAULTS, lds_min_qlen=1, x6_min_qlen=0, lds_waves=4), dict(DEFAULTS, ds_short=0, lds_min_qlen=0)):
                        for ldv in (6 * D, 6 * D + 2):
                            r = route(rt, D, n, max_qlen=max_qlen, ragged=ragged, max_kvlen=max_kvlen, ld=dict(ldv=ldv), **o)
                            kernel, arg = restated(D, max_qlen, n, ragged, max_kvlen, ldv, o)
                            got = {"x6": r["nwq"], "x3h": r["nwq"], "lds": r["nwq"], "ds": r["nkv"], "reg": r["nwv"], "generic": r["nwv"]}
                            assert r["err"] == 0 and (r["kernel"], got[r["kernel"]]) == (kernel, arg), (D, n, max_qlen, ragged, max_kvlen, o, r)
                            qt = r["nwq"]
                            assert r["grid"] == (-(-max_qlen // (32 * qt)), 2, 3)
                            seen.add(kernel)
    assert seen == {"generic", "reg", "ds", "lds", "x6", "x3h"}


# ---- the descriptor ------------------------------------------------------------------------------------------------------------

def test_attention_descriptor_matches_header(rt):
    """ctypes mirror of mt2_attn_desc: same fields in the same order and of the same kind as include/megatts2_hip.h, and of the same
    size - both entry points compare struct_bytes with their own sizeof before they look at anything else (no device needed)."""
    header = open(os.path.join(ROOT, "include", "megatts2_hip.h")).read()
    body = header[header.index("typedef struct mt2_attn_desc {") + len("typedef struct mt2_attn_desc {"):header.index("} mt2_attn_desc;")]
    fields = []
    for decl in body.split(";"):
        decl = decl.strip()
        if not decl:
            continue
        m = re.match(r"(const\s+)?(float|int32_t)\s*(\*)?\s*(.+)$", decl, flags=re.S)
        assert m, decl
        for i, nm in enumerate(m.group(4).split(",")):
            nm = nm.strip()
            ptr = (m.group(3) is not None and i == 0) or nm.startswith("*")
            fields.append((nm.lstrip("* "), "ptr" if ptr else m.group(2)))
    kinds = {"ptr": (ctypes.c_void_p, ctypes.POINTER(ctypes.c_int32)), "int32_t": (ctypes.c_int32,), "float": (ctypes.c_float,)}
    mirror = rt.MT2AttnDesc._fields_
    assert [f[0] for f in fields] == [f[0] for f in mirror]
    for (name, kind), (_, ctype) in zip(fields, mirror):
        assert ctype in kinds[kind], (name, kind, ctype)
    ids = dict(re.findall(r"MT2_ATTN_([A-Z0-9]+) = (\d+)", header))
    assert [k.lower() for k, _ in sorted(ids.items(), key=lambda kv: int(kv[1]))] == list(rt.ATTN_KERNELS)
    lib = rt.load_library()
    d = rt.MT2AttnDesc()
    d.struct_bytes = ctypes.sizeof(rt.MT2AttnDesc)
    kernel = ctypes.c_int32(7)
    d.kernel_out = ctypes.pointer(kernel)
    assert lib.mt2_op_attention_desc(None, ctypes.byref(d)) != 0 and b"bad arguments" in lib.mt2_last_error()
    assert kernel.value == 0
    assert lib.mt2_attention_route(ctypes.byref(d), None, None, None, None, None) == 0
    d.struct_bytes += 8
    assert lib.mt2_op_attention_desc(None, ctypes.byref(d)) != 0 and b"descriptor size mismatch" in lib.mt2_last_error()
    assert lib.mt2_attention_route(ctypes.byref(d), None, None, None, None, None) != 0
    assert lib.mt2_attention_route(None, None, None, None, None, None) != 0
