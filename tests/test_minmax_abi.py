"""CPU: the host side of MIN / MAX by group (plan kind 8) -- the state-word decode helper against numpy, the header and
the Python constants, and the host statement of the re-keying with planes that fold by max."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import exon_amd
from exon_amd import _lib, distributed

import minmax_expect as MX

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "exon_hip.h")).read(), flags=re.S)


def _check_decode(values, is_int):
    y_type = "i32" if is_int else "f32"
    for is_min, word in ((True, MX.min_word), (False, MX.max_word)):
        words = np.concatenate([[0], word(values, is_int), [0]])
        got, valid = exon_amd.minmax_decode(words, is_min, y_type)
        assert got.dtype == (np.int32 if is_int else np.float32)
        assert not valid[0] and not valid[-1] and valid[1:-1].all()
        # bit patterns, not values: NaN payloads and the sign of zero have to survive
        assert np.array_equal(got[1:-1].view(np.uint32), np.ascontiguousarray(values).view(np.uint32))
        # and numpy's own inverse agrees on which words are empty
        assert np.array_equal(MX.decode(words, is_min, is_int)[1], valid)


def test_decode_special_values():
    _check_decode(MX.SPECIAL_F32_BITS.view(np.float32), False)
    _check_decode(MX.SPECIAL_I32, True)


def test_decode_random_bit_patterns():
    bits = np.random.default_rng(8).integers(0, 2**32, 100_000, dtype=np.uint64).astype(np.uint32)
    _check_decode(bits.view(np.float32), False)
    _check_decode(bits.view(np.int32), True)


def test_words_order_like_the_values():
    """the max plane grows with the value and the min plane falls with it -- totalOrder for floats, including the NaNs"""
    order = np.array([0xFFFFFFFF, 0xFFC00000, 0xFF800000, 0xFF7FFFFF, 0x80000001, 0x80000000,
                      0x00000000, 0x00000001, 0x7F7FFFFF, 0x7F800000, 0x7FC00000, 0x7FFFFFFF], np.uint32).view(np.float32)
    assert (np.diff(MX.max_word(order, False)) > 0).all() and (np.diff(MX.min_word(order, False)) < 0).all()
    assert (np.diff(MX.max_word(MX.SPECIAL_I32, True)) > 0).all() and (np.diff(MX.min_word(MX.SPECIAL_I32, True)) < 0).all()
    assert MX.max_word(order, False).min() >= 1 and MX.min_word(order, False).min() >= 1  # 0 stays "no value"
    # the library reads the words the same way: ascending max words and descending min words decode to `order`, bit for bit
    ramp = np.arange(1, 2**32 + 1, 2**32 // 4096 + 1, dtype=np.int64)  # a ramp over the whole word range
    for is_min in (False, True):
        got, valid = exon_amd.minmax_decode((MX.min_word if is_min else MX.max_word)(order, False), is_min, "f32")
        assert valid.all() and np.array_equal(got.view(np.uint32), order.view(np.uint32))
        vals, valid = exon_amd.minmax_decode(ramp, is_min, "i32")
        assert valid.all() and (np.diff(vals.astype(np.int64)) * (-1 if is_min else 1) > 0).all()
        vals, valid = exon_amd.minmax_decode(ramp, is_min, "f32")
        keys = MX.ukey(vals, False).astype(np.int64)  # totalOrder rank of what came out (NaNs at both ends included)
        assert valid.all() and (np.diff(keys) * (-1 if is_min else 1) > 0).all()


def test_decode_rejects_what_is_not_a_state_word():
    lib = exon_amd.load()
    w = np.array([2**32 + 1], np.int64)
    out, valid = np.zeros(1, np.float32), np.zeros(1, np.uint8)
    assert lib.exon_hip_minmax_decode(w.ctypes.data, 1, 0, 0, out.ctypes.data, valid.ctypes.data) == -1
    assert lib.exon_hip_minmax_decode(w.ctypes.data, 1, 0, 7, out.ctypes.data, valid.ctypes.data) == -1
    assert lib.exon_hip_minmax_decode(None, 0, 0, 0, None, None) == 0


def test_header_python_and_abi_version():
    assert re.search(r"#define EXON_HIP_PLAN_CMP_MINMAX_BY_GROUP\s+8\s*$", HEADER, re.M)
    for name in ("exon_hip_cmp_minmax_by_group", "exon_hip_minmax_decode", "exon_hip_plan_fold_states"):
        assert re.search(r"\bint\s+" + name + r"\s*\(", HEADER), name
        assert name in _lib.SIGNATURES and hasattr(exon_amd.load(), name)
    assert _lib.PLAN_CMP_MINMAX_BY_GROUP == 8
    assert exon_amd.load().exon_hip_abi_version() == 5


def test_permute_state_takes_the_max_in_the_extreme_planes():
    import torch
    G = 6
    layout = distributed.state_layout_ex(_lib.PLAN_CMP_MINMAX_BY_GROUP, G)
    assert layout == (G, 4, 0, 0, 2)
    assert distributed.state_layout_ex(_lib.PLAN_CMP_AVG_BY_GROUP, G) == (G, 2, 0, 1, 0)
    assert distributed.state_layout(_lib.PLAN_CMP_AVG_BY_GROUP, G) == (G, 2, 0, 1)  # the four-element form is unchanged
    with pytest.raises(ValueError):
        distributed.state_layout(_lib.PLAN_CMP_MINMAX_BY_GROUP, G)
    y = np.array([1.5, -2.0, 7.25, -0.0], np.float32)
    st = np.zeros(4 * G, np.int64)
    st[0:4] = [3, 1, 2, 5]            # count(y)
    st[G:G + 4] = [4, 1, 2, 6]        # count(*)
    st[2 * G:2 * G + 4] = MX.min_word(y, False)
    st[3 * G:3 * G + 4] = MX.max_word(y + 1, False)
    mapping = [4, 0, 5, 2]            # two sources next to each other land on different targets; targets 1 and 3 get nothing
    out = distributed.permute_state(torch.from_numpy(st), layout, mapping).numpy()
    for p in range(4):
        want = np.zeros(G, np.int64)
        want[mapping] = st[p * G:p * G + 4]
        assert np.array_equal(out[p * G:(p + 1) * G], want), p
    assert not out.reshape(4, G)[:, [1, 3]].any()
    # a dictionary that repeats a name: both sources meet in one target -- counts add, extremes take the max
    out = distributed.permute_state(torch.from_numpy(st), layout, [2, 2, 0, 1]).numpy().reshape(4, G)
    assert out[0, 2] == 4 and out[1, 2] == 5
    assert out[2, 2] == max(st[2 * G], st[2 * G + 1]) and out[3, 2] == max(st[3 * G], st[3 * G + 1])
    assert MX.decode(out[2, 2:3], True, False)[0][0] == -2.0 and MX.decode(out[3, 2:3], False, False)[0][0] == 2.5
