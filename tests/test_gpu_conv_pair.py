"""The fused resblock pair kernel (conv_pair_x3h_kernel, csrc/gemm_x3h.hip) against the two launches of the x3h window kernel that
it replaces, BIT FOR BIT: y = x + conv2(lrelu(conv1(lrelu(x)))) over gap-padded rows, conv1 dilated, conv2 dilation 1.  The row sets
put an utterance boundary at every place of the pair's tile geometry where the two phases could disagree with the two launches."""
import numpy as np
import pytest

from conftest import load_golden, synth_models

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

ACT_NONE, ACT_LRELU = 0, 2
SLOPE = 0.1
SENTINEL = 12345.0
WIN_CFG = {32: 98, 64: 99, 128: 100}            # the x3h window tiles of the two-launch form
BM = {32: 256, 64: 256, 128: 128}
GAP = 4


def row_set(C, k, dil):
    """(valid [R] int32, utterances [(start, end)]) of 600-800 rows for the tile geometry of (C, k): output tiles of bmo rows, conv2's
    halo of (k - 1) / 2 rows and conv1's of (k - 1) / 2 * dil more on either side of a tile."""
    bmo, pad = BM[C] - (k - 1), (k - 1) // 2
    h1 = pad * dil
    utts = []
    a_end = bmo - 1                              # the gap starts inside conv2's halo in front of tile 1
    utts.append((0, a_end))
    b_start = a_end + GAP
    b_end = 2 * bmo - pad - 1                    # ... inside conv1's halo in front of tile 2
    utts.append((b_start, b_end))
    c_start = b_end + GAP
    c_end = 2 * bmo + min(100, bmo // 2)         # a boundary inside tile 2
    utts.append((c_start, c_end))
    d_start = c_end + GAP
    d_end = d_start + max(1, (k - 1) * dil - 1)  # an utterance shorter than conv1's span
    utts.append((d_start, d_end))
    e_start = d_end + GAP
    R = max(640, e_start + 40)
    while R % bmo == 0 or R % bmo > bmo - 8:     # a partial last tile
        R += 1
    utts.append((e_start, R - 2))
    valid = np.zeros(R, np.int32)
    for s, e in utts:
        valid[s:e] = 1
    # what the layout is for
    assert 600 <= R <= 800
    assert bmo - pad <= a_end < bmo                                    # conv2's halo of tile 1
    assert 2 * bmo - pad - h1 <= b_end < 2 * bmo - pad                 # conv1's halo of tile 2
    assert 2 * bmo < c_end < 3 * bmo - pad - h1                        # inside tile 2
    assert 1 <= d_end - d_start < (k - 1) * dil
    assert R % bmo != 0 and not valid[a_end:b_start].any()
    return valid, utts


def operands(C, k, seed, ldx):
    g = torch.Generator().manual_seed(seed)
    K = k * C
    W1 = torch.randn(C, K, generator=g) / np.sqrt(K)
    W2 = torch.randn(C, K, generator=g) / np.sqrt(K)
    b1 = torch.randn(C, generator=g) * 0.1
    b2 = torch.randn(C, generator=g) * 0.1
    return W1, W2, b1, b2


def make_x(valid, C, ldx, seed):
    g = torch.Generator().manual_seed(1000 + seed)
    X = torch.randn(valid.shape[0], ldx, generator=g)
    X[:, :C] *= torch.from_numpy(valid).to(torch.float32)[:, None]      # gap rows of an activation are zeros
    return X.cuda()


def two_launches(rt, X, C, k, dil, W1, W2, b1, b2, valid):
    pad = (k - 1) // 2
    t1, f1 = rt.op_conv_x3h(X, W1.cuda(), b1.cuda(), None, valid, shift0=-pad * dil, taps=k, dil=dil, Cin=C, pro_act=ACT_LRELU,
                            pro_slope=SLOPE, epi_act=ACT_LRELU, force_cfg=WIN_CFG[C], want_flag=True)
    y, f2 = rt.op_conv_x3h(t1, W2.cuda(), b2.cuda(), X, valid, shift0=-pad, taps=k, dil=1, Cin=C, pro_act=ACT_NONE, pro_slope=SLOPE,
                           epi_act=ACT_NONE, force_cfg=WIN_CFG[C], want_flag=True)
    return y, f1, f2


def fused(rt, X, C, k, dil, W1, W2, b1, b2, valid, ldy):
    out = torch.full((X.shape[0], ldy), SENTINEL, device="cuda", dtype=torch.float32)
    y, flag = rt.op_conv_pair(X, W1, b1.cuda(), W2, b2.cuda(), k, dil, SLOPE, valid=valid, channels=C, out=out, want_flag=True)
    return y, flag


def bits(t):
    return t.contiguous().view(torch.int32)


@pytest.fixture(scope="module")
def rt():
    from megatts2_amd import runtime
    return runtime


@pytest.mark.parametrize("C", [32, 64, 128])
@pytest.mark.parametrize("k", [3, 7, 11])
@pytest.mark.parametrize("dil", [1, 3, 5])
def test_pair_is_bit_identical_to_the_two_launches(rt, C, k, dil):
    valid_np, _ = row_set(C, k, dil)
    valid = torch.from_numpy(valid_np).cuda()
    ldx, ldy = C + 8, C + 4
    W1, W2, b1, b2 = operands(C, k, 7 * C + k + dil, ldx)
    X = make_x(valid_np, C, ldx, C + k + dil)
    want, f1, f2 = two_launches(rt, X, C, k, dil, W1, W2, b1, b2, valid)
    got, flag = fused(rt, X, C, k, dil, W1, W2, b1, b2, valid, ldy)
    torch.cuda.synchronize()
    assert torch.equal(bits(got[:, :C]), bits(want))
    assert bool((got[:, C:] == SENTINEL).all())                       # nothing beyond the C columns
    assert not got[:, :C][valid == 0].any()                           # masked rows are written, as zeros
    assert flag == (f1 | f2) == 0


@pytest.mark.parametrize("C", [32, 64, 128])
def test_fewer_rows_than_one_output_tile(rt, C):
    k, dil = 7, 3
    R = 100
    valid_np = np.zeros(R, np.int32)
    valid_np[2:41] = 1
    valid_np[45:97] = 1
    assert R < BM[C] - (k - 1)
    valid = torch.from_numpy(valid_np).cuda()
    W1, W2, b1, b2 = operands(C, k, 5, C)
    X = make_x(valid_np, C, C, 5)
    want, _, _ = two_launches(rt, X, C, k, dil, W1, W2, b1, b2, valid)
    got, flag = fused(rt, X, C, k, dil, W1, W2, b1, b2, valid, C + 4)
    assert torch.equal(bits(got[:, :C]), bits(want))
    assert bool((got[:, C:] == SENTINEL).all()) and flag == 0
    # no row mask at all: every row of [0, R) is an utterance row
    want, _, _ = two_launches(rt, X, C, k, dil, W1, W2, b1, b2, None)
    got, _ = fused(rt, X, C, k, dil, W1, W2, b1, b2, None, C)
    assert torch.equal(bits(got), bits(want))


def test_range_guard_trips_on_t1_exactly_as_in_the_two_launches(rt):
    """conv1's output leaves the fp16 range (a bias of 7e4 on one channel) while h does not: the second launch of the two-launch form
    raises the flag when it splits t1 - so does the pair kernel's second split."""
    C, k, dil = 64, 3, 1
    valid_np, _ = row_set(C, k, dil)
    valid = torch.from_numpy(valid_np).cuda()
    W1, W2, b1, b2 = operands(C, k, 11, C)
    b1[5] = 7.0e4
    X = make_x(valid_np, C, C, 11)
    _, f1, f2 = two_launches(rt, X, C, k, dil, W1, W2, b1, b2, valid)
    _, flag = fused(rt, X, C, k, dil, W1, W2, b1, b2, valid, C)
    assert (f1, f2) == (0, 1)
    assert flag == (f1 | f2)
    # ... and on h itself, in the first split of either form
    X[3, 2] = 7.0e4
    _, f1, f2 = two_launches(rt, X, C, k, dil, W1, W2, torch.zeros(C), b2, valid)
    _, flag = fused(rt, X, C, k, dil, W1, W2, torch.zeros(C), b2, valid, C)
    assert f1 == 1 and flag == (f1 | f2)


def test_tiny_hifigan_waveforms_do_not_change_with_pair_fuse():
    from megatts2_amd import megatts2 as M
    (_, _, _, h), (_, _, _, sd_h) = synth_models("tiny")
    voc = M.HIFIGAN(h, sd_h)
    z = load_golden("tiny_hifigan.npz")
    mels = []
    while f"mel{len(mels)}" in z:
        mels.append(z[f"mel{len(mels)}"])
    n = max(m.shape[0] for m in mels)
    mel = np.zeros((len(mels), n, mels[0].shape[1]), np.float32)
    for i, m in enumerate(mels):
        mel[i, :m.shape[0]] = m
    lens = np.asarray([m.shape[0] for m in mels], np.int32)
    x = torch.from_numpy(mel).cuda().transpose(1, 2).contiguous()
    wav = {}
    for mask in (7, 0):
        voc.native.set_option("pair_fuse", mask)
        wav[mask] = voc.decode_batch(x, mel_lens=lens).cpu().numpy()
    assert wav[0].any()
    assert np.array_equal(wav[7], wav[0])
