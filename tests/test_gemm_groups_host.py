"""Host side of grouped GEMM launches (no GPU): the rule by which a launch walks the fp16 planes of a weight buffer
(csrc/x3h_planes.h x3h_group_planes - what model_stages.hip attach_planes applies and what runtime.op_gemm_grouped derives its strides
from), against a restatement in plain Python; and the ctypes mirror of the grouped-launch descriptor."""
import ctypes
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def rt():
    from megatts2_amd import runtime
    return runtime


def padded_k(row_len):
    """x3h_padded_k: a plane row holds whole 32-k chunks."""
    return -(-row_len // 32) * 32


def restated(row_len, w_off, ldw, strideW, groups):
    """The rule, written from its description: the planes carry one scale per row of the [rows][row_len] matrix they were split
    by and store a row as blocks of 128 bytes per 32 k.  A launch can use them when it walks the buffer with those rows (ldw ==
    row_len) and starts on a block; its groups then step through whole matrices ("whole": strideW is a multiple of the row length,
    rows and scales move together) or through K slices inside ONE row ("slices": blocks move, scales are shared); one group needs
    neither."""
    row0, col0 = divmod(w_off, row_len)
    ldb = 4 * padded_k(row_len)
    if ldw != row_len or col0 % 32:
        return None
    whole = strideW % row_len == 0
    slices = (not whole) and col0 + strideW * groups <= row_len and strideW % 32 == 0
    if not (whole or slices or groups == 1):
        return None
    out = {"form": "whole" if whole else "slices", "wh_off": row0 * ldb + (col0 // 32) * 128, "wh_ldb": ldb, "inv_off": row0}
    if whole:
        out["wh_gstride"], out["wh_inv_stride"] = (strideW // row_len) * ldb, strideW // row_len
    else:
        out["wh_gstride"], out["wh_inv_stride"] = (strideW // 32) * 128, 0
    return out


# (row_len, w_off, ldw, strideW, groups) -> what the launch gets, spelled out where it matters
CASES = [
    # whole matrices: the parallel branches of a conv stack, 96 rows of 5 * 64 each, starting at the second stack entry
    ("whole", (320, 3 * 96 * 320, 320, 96 * 320, 3),
     {"form": "whole", "wh_off": 288 * 1280, "wh_ldb": 1280, "wh_gstride": 96 * 1280, "inv_off": 288, "wh_inv_stride": 96}),
    # shared weights: a stride of 0 is a multiple of every row length
    ("shared", (320, 0, 320, 0, 3),
     {"form": "whole", "wh_off": 0, "wh_ldb": 1280, "wh_gstride": 0, "inv_off": 0, "wh_inv_stride": 0}),
    # K slices inside one row: split-K, four slices of 256 of K = 1024, starting at row 16
    ("slices", (1024, 16 * 1024, 1024, 256, 4),
     {"form": "slices", "wh_off": 16 * 4096, "wh_ldb": 4096, "wh_gstride": 1024, "inv_off": 16, "wh_inv_stride": 0}),
    # ... starting inside the row (the second half of K in two slices)
    ("slices at a column", (1024, 16 * 1024 + 512, 1024, 256, 2),
     {"form": "slices", "wh_off": 16 * 4096 + 16 * 128, "wh_ldb": 4096, "wh_gstride": 1024, "inv_off": 16, "wh_inv_stride": 0}),
    # a stride that is neither a multiple of the row length nor inside one row: the third slice leaves the row
    ("slices leave the row", (1024, 512, 1024, 256, 3), None),
    ("stride across rows", (1024, 0, 1024, 1024 + 256, 2), None),
    # a launch that starts inside a 32-k block
    ("col0 % 32", (1024, 16, 1024, 0, 1), None),
    ("col0 % 32, groups", (1024, 1024 + 8, 1024, 256, 2), None),
    # slices that are no whole blocks
    ("strideW % 32", (1024, 0, 1024, 48, 4), None),
    # a launch that walks the buffer with another row length
    ("ldw != row_len", (1024, 0, 512, 0, 1), None),
    ("ldw != row_len, groups", (320, 0, 640, 96 * 320, 3), None),
    # one group at a row offset (and at a column): the pointer alone moves
    ("one group at a row", (768, 40 * 768, 768, 0, 1),
     {"form": "whole", "wh_off": 40 * 3072, "wh_ldb": 3072, "wh_gstride": 0, "inv_off": 40, "wh_inv_stride": 0}),
    ("one group at a row and column", (768, 40 * 768 + 256, 768, 0, 1),
     {"form": "whole", "wh_off": 40 * 3072 + 8 * 128, "wh_ldb": 3072, "wh_gstride": 0, "inv_off": 40, "wh_inv_stride": 0}),
    # one group whose (unused) stride is neither form: still served, the group stride stays on whole blocks
    ("one group, odd stride", (768, 0, 768, 100, 1),
     {"form": "slices", "wh_off": 0, "wh_ldb": 3072, "wh_gstride": 3 * 128, "inv_off": 0, "wh_inv_stride": 0}),
    # a row length that is no multiple of 32: plane rows are padded to whole chunks (x3h_padded_k), f32 rows are not
    ("padded rows", (104, 5 * 104, 104, 7 * 104, 3),
     {"form": "whole", "wh_off": 5 * 512, "wh_ldb": 512, "wh_gstride": 7 * 512, "inv_off": 5, "wh_inv_stride": 7}),
    ("padded rows, K = 7 * 20", (140, 0, 140, 96 * 140, 2),
     {"form": "whole", "wh_off": 0, "wh_ldb": 640, "wh_gstride": 96 * 640, "inv_off": 0, "wh_inv_stride": 96}),
]


@pytest.mark.parametrize("name,args,want", CASES, ids=[c[0] for c in CASES])
def test_plane_stride_rule_matches_its_restatement(rt, name, args, want):
    got = rt.x3h_group_planes(*args)
    assert got == restated(*args), (name, got)
    assert got == want, (name, got)            # and the restatement itself says what the case was written for
    if got is not None:                        # what the engine asks of the planes: whole 128-byte blocks
        assert got["wh_off"] % 128 == 0 and got["wh_ldb"] % 128 == 0 and got["wh_gstride"] % 128 == 0
        assert got["wh_ldb"] == 4 * padded_k(args[0])


def test_plane_stride_rule_on_a_grid_of_launches(rt):
    """Every combination of a few row lengths, offsets, strides and group counts: the library and the restatement agree (the
    explicit expectations of CASES are what is independent of both), and what is served has the properties the kernels rely on:
    whole 128-byte blocks, group g's planes and scales inside the rows the launch owns."""
    n = served = 0
    for row_len in (32, 104, 256, 1024):
        for w_off in (0, 32, 48, row_len, 3 * row_len + 64, 5 * row_len + 8):
            for ldw in (row_len, 2 * row_len):
                for strideW in (0, 32, 48, 256, row_len, row_len + 32, 16 * row_len):
                    for groups in (1, 2, 3, 4):
                        got = rt.x3h_group_planes(row_len, w_off, ldw, strideW, groups)
                        assert got == restated(row_len, w_off, ldw, strideW, groups), (row_len, w_off, ldw, strideW, groups)
                        n += 1
                        served += got is not None
                        if got is None:
                            continue
                        assert got["wh_off"] % 128 == 0 and got["wh_gstride"] % 128 == 0 and got["wh_ldb"] == 4 * padded_k(row_len)
                        # the first element of group g, (row, column) in the f32 buffer, is where its planes and its scale are
                        for g in range(groups if groups > 1 else 1):
                            row, col = divmod(w_off + g * strideW, row_len)
                            assert got["wh_off"] + g * got["wh_gstride"] == row * got["wh_ldb"] + (col // 32) * 128
                            assert got["inv_off"] + g * got["wh_inv_stride"] == row
    assert 0 < served < n


def test_plane_stride_rule_rejects_bad_arguments(rt):
    for args in ((0, 0, 0, 0, 1), (32, -1, 32, 0, 1), (32, 0, 32, 0, 0)):
        with pytest.raises(rt.NativeError, match="bad arguments"):
            rt.x3h_group_planes(*args)


def test_grouped_descriptor_matches_header(rt):
    """ctypes mirror of mt2_gemm_desc: same fields in the same order and of the same kind as include/megatts2_hip.h."""
    header = open(os.path.join(ROOT, "include", "megatts2_hip.h")).read()
    body = header[header.index("typedef struct mt2_gemm_desc {") + len("typedef struct mt2_gemm_desc {"):header.index("} mt2_gemm_desc;")]
    fields = []
    for decl in body.split(";"):
        decl = decl.strip()
        if not decl:
            continue
        m = re.match(r"(const\s+)?(float|void|int32_t|long long)\s*(\*)?\s*(.+)$", decl, flags=re.S)
        assert m, decl
        base, names = m.group(2), m.group(4)
        for i, nm in enumerate(names.split(",")):
            nm = nm.strip()
            ptr = (m.group(3) is not None and i == 0) or nm.startswith("*")
            kind = "ptr" if ptr else base
            fields.append((nm.lstrip("* "), kind))
    kinds = {"ptr": (ctypes.c_void_p, ctypes.POINTER(ctypes.c_int32)), "int32_t": (ctypes.c_int32,), "float": (ctypes.c_float,),
             "long long": (ctypes.c_longlong,)}
    mirror = rt.MT2GemmDesc._fields_
    assert [f[0] for f in fields] == [f[0] for f in mirror]
    for (name, kind), (_, ctype) in zip(fields, mirror):
        assert ctype in kinds[kind], (name, kind, ctype)
    # ... and of the same size: the entry point compares struct_bytes with its own sizeof before it looks at anything else (no
    # device needed: an empty descriptor of the right size gets as far as the argument check, one of another size does not)
    lib = rt.load_library()
    d = rt.MT2GemmDesc()
    d.struct_bytes = ctypes.sizeof(rt.MT2GemmDesc)
    assert lib.mt2_op_gemm_grouped(None, ctypes.byref(d)) != 0 and b"bad arguments" in lib.mt2_last_error()
    d.struct_bytes += 8
    assert lib.mt2_op_gemm_grouped(None, ctypes.byref(d)) != 0 and b"descriptor size mismatch" in lib.mt2_last_error()
