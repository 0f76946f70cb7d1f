"""The bf16 gather of the XCD-local SpMM, host side (no GPU): include/dgmi_bf16.h declares exactly the new entry points,
the library exports them and the fifth ctypes table matches; the four older headers and the ABI version are what they
were; the torch ops are registered; argument validation returns codes / raises before any launch; the
``gather_precision`` default nests, restores and is local to its thread."""
import hashlib
import os
import re
import threading

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY_POINTS = ["dgmi_rows_to_bf16", "dgmi_spmm_sliced_bf16"]
# sha256 of the pinned headers: the bf16 entry points were added WITHOUT touching them (dgmi.h: re-pinned after one comment
# sentence on finite edge weights was added to the edge-dropout paragraph, and again after one on zero rows was added to the
# kNN paragraph, and again after one on the key bits `dgmi_csr_sliced_from_csr_i32` admits, and again after one on the NaN-keeping relu
# of `dgmi_gather_add_f32`, and again after the non-finite contract was added to the kNN paragraph; no declaration changed)
PINNED = {
    "dgmi.h": "07cc4abb82fbd1fd66b8a314ac613af6ced1cf9f4ef487dea9e480a56148c306",
    "dgmi_pairs.h": "9911f584a90f5b340c7d3cfe009e71d17b431dedc7f3817f687c6c4ef2b3ca4f",
    "dgmi_rank.h": "d7333eb8cf8e95e9bbaa5ad2e7ffced95ebc89617e249009e25988cf854da931",
    "dgmi_above.h": "76600e1650a703f70f44f841706e331aa9871f7f18cf07ca3bf4a0b7a5595aea",
}


def _text(name="dgmi_bf16.h"):
    return open(os.path.join(ROOT, "include", name)).read()


def _prototypes():
    return {m.group(1): m.group(2) for m in re.finditer(r"DGMI_API\s+[\w\s\*]+?\b(dgmi_\w+)\s*\(([^)]*)\)\s*;", _text())}


def test_header_declares_the_bf16_entry_points():
    assert sorted(_prototypes()) == ENTRY_POINTS
    assert '#include "dgmi.h"' in _text()


def test_the_older_headers_and_the_abi_version_are_unchanged():
    from dream_gnn_amd import _lib

    for name, digest in PINNED.items():
        assert hashlib.sha256(_text(name).encode()).hexdigest() == digest, name
        assert not any(e in _text(name) for e in ENTRY_POINTS), name
    assert _lib.ABI_VERSION == 20 and _lib.lib.dgmi_abi_version() == 20
    assert "#define DGMI_ABI_VERSION 20" in _text("dgmi.h")


def test_library_exports_the_bf16_entry_points():
    from dream_gnn_amd import _lib

    assert sorted(_lib.BF16_SIGNATURES) == ENTRY_POINTS
    for other in (_lib.SIGNATURES, _lib.PAIR_SIGNATURES, _lib.RANK_SIGNATURES, _lib.ABOVE_SIGNATURES):
        assert not set(_lib.BF16_SIGNATURES) & set(other)
    protos = _prototypes()
    ctype_of = {"int64_t": "c_long", "int32_t": "c_int", "float": "c_float", "size_t": "c_ulong", "dgmi_stream_t": "c_void_p"}
    for name, (res, args) in _lib.BF16_SIGNATURES.items():
        fn = getattr(_lib.lib, name)
        assert fn.restype is res and list(fn.argtypes) == args, name
        params = [p.strip() for p in protos[name].split(",")]
        assert len(params) == len(args), name
        for p, a in zip(params, args):
            assert a.__name__ == ("c_void_p" if "*" in p else ctype_of[p.split()[0]]), (name, p)
    # the argument list of dgmi_spmm_sliced_f32 minus src_scale
    f32 = re.search(r"dgmi_spmm_sliced_f32\s*\(([^)]*)\)\s*;", _text("dgmi.h")).group(1)
    names = lambda proto: [p.split()[-1].lstrip("*") for p in proto.split(",")]
    assert names(protos["dgmi_spmm_sliced_bf16"]) == [n for n in names(f32) if n != "src_scale"]
    assert "const uint16_t* X" in protos["dgmi_spmm_sliced_bf16"]


def _convert(L, **kw):
    a = dict(X=16, ldx=136, scale=None, n=10, F=136, out=32, ldo=136, stream=None)
    a.update(kw)
    return L.dgmi_rows_to_bf16(a["X"], a["ldx"], a["scale"], a["n"], a["F"], a["out"], a["ldo"], a["stream"])


def _spmm(L, **kw):
    a = dict(segptr=16, indices=16, vals=None, eid=None, keep=None, n_keep=0, X=16, ldx=128, ds=None, Y=32, ldy=128, n_dst=4,
             n_src=4, F=128, n_slices=8, passes=0, mult=0, planes=48, pbytes=1 << 30, act=0, slope=0.0, mask=None, ldm=0,
             mscale=1.0, stream=None)
    a.update(kw)
    return L.dgmi_spmm_sliced_bf16(a["segptr"], a["indices"], a["vals"], a["eid"], a["keep"], a["n_keep"], a["X"], a["ldx"],
                                   a["ds"], a["Y"], a["ldy"], a["n_dst"], a["n_src"], a["F"], a["n_slices"], a["passes"],
                                   a["mult"], a["planes"], a["pbytes"], a["act"], a["slope"], a["mask"], a["ldm"], a["mscale"],
                                   a["stream"])


def test_argument_validation_returns_codes_without_a_gpu():
    from dream_gnn_amd import _lib

    L = _lib.lib
    # the conversion pass
    assert _convert(L, n=0) == 0 and _convert(L, F=0, ldx=0, ldo=0) == 0 and _convert(L, n=0, X=None, out=None) == 0
    assert _convert(L, F=132, ldx=132) == -1 and _convert(L, F=4, ldx=8, ldo=8) == -1      # F % 8
    assert _convert(L, ldx=128) == -1 and _convert(L, ldo=128) == -1                       # ld < F
    assert _convert(L, ldx=138) == -1 and _convert(L, ldo=140) == -1                       # ldx % 4, ldo % 8
    assert _convert(L, X=20) == -1 and _convert(L, out=40) == -1                           # 16-B alignment
    assert _convert(L, X=None) == -1 and _convert(L, out=None) == -1 and _convert(L, n=-1) == -1
    assert _convert(L, X=32, out=32) == -1                                                  # in place
    assert _convert(L, F=2 ** 31 + 8, ldx=2 ** 31 + 8, ldo=2 ** 31 + 8) == -2
    # the product
    assert _spmm(L, n_dst=0) == 0 and _spmm(L, F=0, ldx=0, ldy=0) == 0
    assert _spmm(L, F=124, ldx=128) == -1 and _spmm(L, F=4, ldx=8, ldy=4) == -1            # F % 8 (F % 4 is not enough)
    assert _spmm(L, ldx=132) == -1 and _spmm(L, ldx=120) == -1 and _spmm(L, ldy=130) == -1 and _spmm(L, ldy=64) == -1
    assert _spmm(L, X=24) == -1 and _spmm(L, Y=40) == -1 and _spmm(L, planes=56) == -1     # 16-B alignment
    assert _spmm(L, X=None) == -1 and _spmm(L, Y=None) == -1 and _spmm(L, planes=None) == -1 and _spmm(L, segptr=None) == -1
    assert _spmm(L, X=32, Y=32) == -1                                                       # Y aliases X
    assert _spmm(L, passes=2) == -1 and _spmm(L, mult=2) == -1 and _spmm(L, n_slices=0) == -1 and _spmm(L, n_slices=65) == -1
    assert _spmm(L, vals=16, mult=1) == -1                                                  # values AND multiplicities
    assert _spmm(L, n_keep=1) == -1 and _spmm(L, n_keep=9, eid=16, keep=16) == -1           # keep without eid; > 8 descriptions
    assert _spmm(L, act=2) == -1 and _spmm(L, mask=16, ldm=64) == -1 and _spmm(L, mask=20, ldm=128) == -1
    assert _spmm(L, n_dst=2 ** 31) == -2 and _spmm(L, n_src=2 ** 31) == -2
    assert _spmm(L, pbytes=0) == -3                                                         # planes too small
    assert _spmm(L, pbytes=L.dgmi_spmm_sliced_planes_bytes(4, 8, 128) - 1) == -3          # sized by the fp32 product's query


def test_torch_ops_are_registered_for_the_device_only():
    from dream_gnn_amd import _lib  # noqa: F401

    T = torch.ops.dreamgnn_mi
    assert [a.name for a in T.rows_to_bf16.default._schema.arguments] == ["X", "scale"]
    raw = [a.name for a in T.spmm_sliced_bf16_raw.default._schema.arguments]
    f32 = [a.name for a in T.spmm_sliced_raw.default._schema.arguments]
    assert raw == [n for n in f32 if n != "src_scale"]
    out = [a.name for a in T.spmm_sliced_bf16_out.default._schema.arguments]
    assert out == [n for n in (a.name for a in T.spmm_sliced_out.default._schema.arguments) if n != "src_scale"]
    with pytest.raises(NotImplementedError):  # no CPU kernel
        T.rows_to_bf16(torch.zeros(2, 8), None)
    with pytest.raises(NotImplementedError):
        T.spmm_sliced_bf16_raw(torch.zeros(9, dtype=torch.int32), torch.zeros(0, dtype=torch.int32), None, None, None,
                               torch.zeros(1, 8, dtype=torch.bfloat16), None, 1, 8)


def _host_layout():
    """A SlicedCSR that never saw a device: enough for the checks that come before the first launch."""
    from dream_gnn_amd import ops

    sl = ops.SlicedCSR.__new__(ops.SlicedCSR)
    sl.n_dst, sl.n_src, sl.n_slices = 1, 3, 8
    sl.segptr, sl.indices = torch.zeros(9, dtype=torch.int32), torch.zeros(0, dtype=torch.int32)
    sl.eid = sl.vals = None
    sl.id_mult = False
    return sl


def test_ops_validate_before_the_device():
    import dream_gnn_amd
    from dream_gnn_amd import ops

    assert dream_gnn_amd.gather_precision is ops.gather_precision and "gather_precision" in dream_gnn_amd.__all__
    sl = _host_layout()
    with pytest.raises(RuntimeError, match="pass the float32 table"):  # bf16 + src_scale: refused before the device check
        sl.spmm(torch.zeros(3, 8, dtype=torch.bfloat16), src_scale=torch.ones(3))
    with pytest.raises(RuntimeError, match="MI355X only"):
        sl.spmm(torch.zeros(3, 8, dtype=torch.bfloat16))
    with pytest.raises(RuntimeError, match="MI355X only"):
        ops.rows_to_bf16(torch.zeros(3, 8))
    with pytest.raises(ValueError, match="gather_dtype"):
        sl.spmm(torch.zeros(3, 8), gather_dtype=torch.float16)
    with pytest.raises(ValueError, match="gather_dtype"):
        ops.spmm_csr(None, torch.zeros(3, 8), gather_dtype=torch.float64)
    with pytest.raises(ValueError, match="gather_dtype"):
        with ops.gather_precision(torch.int8):
            pass


def test_gather_precision_nests_restores_and_is_thread_local():
    from dream_gnn_amd import ops

    bf16, f32 = torch.bfloat16, torch.float32
    R = ops._resolve_gather_dtype
    assert R(None) is f32 and R(bf16) is bf16 and R(f32) is f32
    with ops.gather_precision(bf16):
        assert R(None) is bf16 and R(f32) is f32  # an explicit keyword wins
        with ops.gather_precision(f32):
            assert R(None) is f32
            with ops.gather_precision(None):
                assert R(None) is f32
            assert R(None) is f32
        assert R(None) is bf16
        seen = {}
        t = threading.Thread(target=lambda: seen.update(inner=R(None)))
        t.start()
        t.join()
        assert seen["inner"] is f32  # another thread keeps its own default

        def other():
            with ops.gather_precision(f32):
                seen["other"] = R(None)

        t = threading.Thread(target=other)
        t.start()
        t.join()
        assert seen["other"] is f32 and R(None) is bf16  # ... and cannot change this one's
    assert R(None) is f32
    with pytest.raises(KeyError):
        with ops.gather_precision(bf16):
            raise KeyError("restored on the way out of an exception")
    assert R(None) is f32
