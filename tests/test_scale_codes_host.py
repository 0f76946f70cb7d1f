"""The coded id words of the owned form's scaled product (``ops.CSRGraph.scale_codes``, include/dgmi_scale.h) on the host:
``table[(word >> 17) & 2047]`` is the scale of the word's source bit for bit, the id and the multiplicity field survive,
the bounds (2048 bit patterns, 2^17 ids) are enforced, and the constants, the header and the ctypes table agree."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHIFT, BITS = 17, 11


def _words(n_src, E, seed, with_mult):
    rng = np.random.default_rng(seed)
    ids = rng.integers(0, n_src, E).astype(np.int32)
    ids[:2] = (0, n_src - 1)
    mult = rng.integers(0, 8, E).astype(np.int32) if with_mult else np.zeros(E, np.int32)
    return torch.from_numpy(ids), torch.from_numpy(mult), torch.from_numpy(ids | (mult << 28))


@pytest.mark.parametrize("with_mult", [False, True])
@pytest.mark.parametrize("n_src,n_values", [(1, 1), (330, 37), (5000, 2048), (1 << SHIFT, 2048)])
def test_decoding_reproduces_the_scale_of_every_edge(n_src, n_values, with_mult):
    from dream_gnn_amd import ops

    rng = np.random.default_rng(n_src)
    values = rng.standard_normal(n_values).astype(np.float32)
    assert np.unique(values.view(np.int32)).size == n_values
    s = values[np.arange(n_src) % n_values]
    ids, mult, words_in = _words(n_src, 20000, 3, with_mult)
    table, words = ops.CSRGraph.scale_codes(torch.from_numpy(s), words_in)
    assert table.dtype == torch.float32 and table.numel() == n_values and words.dtype == torch.int32
    code = (words >> SHIFT) & ((1 << BITS) - 1)
    assert torch.equal(table[code.long()].view(torch.int32), torch.from_numpy(s)[ids.long()].view(torch.int32))
    assert torch.equal(words & ((1 << SHIFT) - 1), ids)
    assert torch.equal((words >> 28) & 7, mult) and bool((words >= 0).all())  # bit 31 stays clear
    assert torch.equal(words_in, torch.from_numpy(ids.numpy() | (mult.numpy() << 28)))  # the input is left alone


def test_every_bit_pattern_keeps_a_code_of_its_own():
    from dream_gnn_amd import ops

    bits = np.array([0x00000000, 0x80000000, 0x7FC00000, 0x7FC00123, 0xFFC00000, 0x7F800000, 0xFF800000, 0x3F800000], np.uint32)
    s = np.tile(bits, 3).view(np.float32)
    ids = torch.arange(s.size, dtype=torch.int32)
    table, words = ops.CSRGraph.scale_codes(torch.from_numpy(s), ids)
    assert table.numel() == bits.size
    got = table[((words >> SHIFT) & 2047).long()].view(torch.int32)
    assert torch.equal(got, torch.from_numpy(s).view(torch.int32))


def test_the_bounds_are_enforced():
    from dream_gnn_amd import ops

    ids = torch.zeros(4, dtype=torch.int32)
    s = torch.arange(5000, dtype=torch.float32)
    assert ops.CSRGraph.scale_codes(s % 2049, ids) == (None, None)
    table, _ = ops.CSRGraph.scale_codes(s % 2048, ids)
    assert table.numel() == 2048
    assert ops.CSRGraph.scale_codes(torch.ones(1 << SHIFT), ids)[0].numel() == 1
    with pytest.raises(RuntimeError, match="at most 131072"):
        ops.CSRGraph.scale_codes(torch.ones((1 << SHIFT) + 1), ids)
    with pytest.raises(RuntimeError):
        ops.CSRGraph.scale_codes(torch.ones(8, dtype=torch.float64), ids)


def test_constants_header_and_binding_agree():
    from dream_gnn_amd import _lib, ops

    header = open(os.path.join(ROOT, "include", "dgmi_scale.h")).read()
    kernels = open(os.path.join(ROOT, "dream_gnn_amd", "csrc", "dgmi_kernels.h")).read()
    assert int(re.search(r"#define DGMI_SCALE_CODE_SHIFT (\d+)", header).group(1)) == SHIFT == ops.SCALE_SHIFT
    assert int(re.search(r"#define DGMI_SCALE_CODE_BITS (\d+)", header).group(1)) == BITS == ops.SCALE_BITS
    assert int(re.search(r"constexpr int kScaleShift = (\d+);", kernels).group(1)) == SHIFT
    assert int(re.search(r"constexpr int kScaleBits = (\d+);", kernels).group(1)) == BITS
    assert SHIFT + BITS == ops.MULT_SHIFT and ops.SCALE_MAX_IDS == 1 << SHIFT and ops.SCALE_MAX_CODES == 1 << BITS
    declared = sorted(re.findall(r"DGMI_API\s+\w+\s+(dgmi_\w+)\(", header))
    assert declared == sorted(_lib.SCALE_SIGNATURES) == ["dgmi_spmm_owned_scaled_f32", "dgmi_spmm_owned_scaled_takes"]
    for name in declared:
        assert hasattr(_lib.lib, name)
        n_args = len(re.search(name + r"\((.*?)\);", header, re.S).group(1).split(","))
        assert n_args == len(_lib.SCALE_SIGNATURES[name][1]), name
    for other in (_lib.SIGNATURES, _lib.PAIR_SIGNATURES, _lib.RANK_SIGNATURES, _lib.ABOVE_SIGNATURES, _lib.BF16_SIGNATURES,
                  _lib.GIVEN_SIGNATURES, _lib.CURVE_SIGNATURES, _lib.LAYOUT_SIGNATURES, _lib.TRAIN_SIGNATURES, _lib.ATTN_SIGNATURES):
        assert not set(_lib.SCALE_SIGNATURES) & set(other)


def test_the_host_query_and_the_argument_checks_need_no_device():
    """``dgmi_spmm_owned_scaled_takes`` is host arithmetic (with a forced grid no device is asked for its CUs), and the
    entry point returns its argument errors, and declines an empty product, before anything is launched."""
    from dream_gnn_amd import _lib

    knobs = dict(sliced_owned=1, sliced_owned_grid=3, sliced_lpr=32)
    try:
        for k, v in knobs.items():
            _lib.set_tuning(k, v)
        takes = lambda n_src=330, n=37, **kw: _lib.owned_scaled_takes(301, n_src, 128, 128, 16, kw.get("mult", False), n)
        assert takes() and takes(mult=True) and takes(n_src=1 << SHIFT, n=1 << BITS)
        assert not takes(n_src=(1 << SHIFT) + 1) and not takes(n=(1 << BITS) + 1) and not takes(n=0)
        _lib.set_tuning("sliced_lpr", 64)
        assert not takes()
        _lib.set_tuning("sliced_lpr", 32)
        _lib.set_tuning("sliced_owned_scaled", 0)
        assert not takes()
        _lib.set_tuning("sliced_owned_scaled", -1)
        _lib.set_tuning("sliced_owned", 0)
        assert not takes()
    finally:
        for k, v in dict(sliced_owned=-1, sliced_owned_grid=0, sliced_lpr=0, sliced_owned_scaled=-1).items():
            _lib.set_tuning(k, v)
    taken = ctypes.c_int32(7)
    f = _lib.lib.dgmi_spmm_owned_scaled_f32
    assert f(None, None, None, 128, None, 1, None, None, 128, 0, 330, 128, 16, 0, 0, 0.0, None, 0, 1.0, ctypes.byref(taken), None) == 0
    assert taken.value == 0  # an empty product: declined
    assert f(None, None, None, 128, None, 1, None, None, 128, 301, 330, 128, 16, 0, 0, 0.0, None, 0, 1.0, ctypes.byref(taken), None) != 0
    assert f(None, None, None, 128, None, 1, None, None, 128, 301, 330, 128, 16, 0, 0, 0.0, None, 0, 1.0, None, None) != 0
