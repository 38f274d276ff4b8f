"""Where the flat leaf-box loop reads: terra_amd_leaf_box_offsets, the byte offsets csrc/dev_types.h gives the device code, against the same layout restated
here. No GPU needed.

What this pins and what it does not: the constants (entry size, pad words, strides), that a table of 1..32 boxes stays inside the entries and property records
its launch stages, that no two slots share a word, and that every box is a 16-bit immediate away from box 0. It does NOT see what make_tracer stores: the link
from these offsets to its stores is a set of static_asserts on the same constants, and an entry index in make_tracer that stopped being slot 6 k + 2 a + s
would pass here. Only the device tests (tests/test_flat_loop_layout_gpu.py, tests/test_leaf_boxes_gpu.py: frames bit for bit) catch that.

The layout: make_tracer (csrc/render_kernels.hip) stages the six permuted copies of the triangles as 48-byte entries, c[kz] triangle p0 p1 at the end of each,
and counts the entries through the copies: entry 6 k + 2 a + s carries box k, axis a, (min, max) for s = 0 and (max, min) for s = 1 in its last two words. Box
k's mask is the last word of the k-th 64-byte staged property record."""
import ctypes as C

import numpy as np
import pytest

from terra_amd import runtime

ENTRY, PAD_WORDS_AT, PROPS, PROPS_PAD_AT = 48, 40, 64, 60
MAX_BOXES = 32


@pytest.fixture(scope="module")
def offsets(amd_lib):
    L = runtime.load(need_torch=False)
    f = L.fn("terra_amd_leaf_box_offsets", C.c_int, [C.c_uint32, C.POINTER(C.c_uint32), C.POINTER(C.c_uint32)])

    def call(n):
        planes = (C.c_uint32 * (6 * n))(); masks = (C.c_uint32 * n)()
        reach = f(n, planes, masks)
        return reach, np.array(planes, dtype=np.int64).reshape(n, 3, 2), np.array(masks, dtype=np.int64)
    call.raw = f; call.lib = L
    return call


@pytest.mark.parametrize("n", range(1, MAX_BOXES + 1))
def test_offsets_are_the_pad_words_make_tracer_fills(offsets, n):
    reach, planes, masks = offsets(n)
    for k in range(n):
        for a in range(3):
            for s in range(2):
                assert planes[k, a, s] == ENTRY * (6 * k + 2 * a + s) + PAD_WORDS_AT, (k, a, s)
        assert masks[k] == PROPS * k + PROPS_PAD_AT
    # the 8 bytes of a pair are an entry's last two words and nothing else; no two slots share a word
    assert ((planes % ENTRY) == ENTRY - 8).all() and len(set(planes.ravel().tolist())) == 6 * n
    # every entry a table of n boxes touches exists: a scene stages at least n triangles, 6 n entries (terra_leaf_boxes_fit)
    assert planes.max() + 8 <= ENTRY * 6 * n and masks.max() + 4 <= PROPS * n
    # the loop's immediates: box k from box 0, same axis and sign; the largest one is what the call returns
    imm = planes - planes[0]
    assert (imm == imm[:, :1, :1]).all() and reach == imm.max() == 6 * ENTRY * (n - 1)
    assert reach + 8 <= 1 << 16


def test_the_largest_table_fits_the_immediate_and_larger_ones_are_refused(offsets):
    reach, planes, masks = offsets(MAX_BOXES)
    assert reach == 8928 and reach < 1 << 16
    assert offsets.raw(MAX_BOXES + 1, None, None) < 0 and "at most" in runtime.last_error()
    offsets.lib.clear_error()
    assert offsets.raw(0, None, None) == 0
