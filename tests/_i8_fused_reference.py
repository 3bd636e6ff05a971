"""The yardstick of the int8 GEMM's operand-out epilogue (include/lq_hip.h, lq_i8_gemm_quantize): the composition of functions
tests/_i8_reference.py already has,

    pack_layout(operand_of_activation(act(gemm_reference(a, b, bias)), 64))

Only ``act``, the case table and the planted cases live here.  tests/test_i8_fused_cpu.py asserts the data conditions of these
inputs on the reference alone; tests/test_gpu_i8_fused.py compares the device with it byte for byte."""
import numpy as np

import _i8_reference as R

OUT_BLOCK = 64
MIN_SCALE = np.float32(2.0 ** -126)

# (M, N, K, a_block, b_block).  (1, 1, 1): the smallest case.  (16, 64, 64): one wave, one instruction, nothing masked.  (17, 65, 65):
# a second row tile with one live line, a second column block with one live column (three of its four tiles clamped copies), a
# second K step with one live k.  (33, 10, 784): the MNIST layer's K under one-step periods of A; N below a block, three clamped
# tiles.  (70, 130, 200): two thread blocks along m (the second with 6 live lines in its one tile), three along n (the last with two
# live columns), periods of one step with B's scale changing every second one, a short last period.  (64, 128, 128): whole tiles
# everywhere, a_every = 2 -- but K = 128 under a_block = 128 is ONE scale block of A: its scale never changes, and ia is advanced
# only after the last read (a scale of A that does change under a_every >= 2 is tests/_matrix_forms.py's NEW_I8_FUSED).
# (100, 192, 256): periods of two steps, a last row tile of 4 lines.  (31, 63, 192): 15 live lines in the last tile, N one below a
# block, periods of two steps.
CASES = [(1, 1, 1, 0, 0), (16, 64, 64, 0, 0), (17, 65, 65, 0, 0), (33, 10, 784, 64, 0), (70, 130, 200, 64, 128), (64, 128, 128, 128, 64),
         (100, 192, 256, 0, 128), (31, 63, 192, 128, 0)]
# Every case is _i8_reference.gemm_case's seed 0; for (1, 1, 1) it gives Y > 0 with and without the bias, so relu does not empty the
# operand (tests/test_i8_fused_cpu.py asserts it).
# The cases with too few outputs for 60 distinct code values, and the number asked of them instead: (1, 1, 1) has one output;
# (33, 10, 784) has 330, about half of them +0 under relu, and the rest cannot be asked for more than 40 values
DEGENERATE = {((1, 1, 1, 0, 0), None): 1, ((1, 1, 1, 0, 0), "relu"): 1, ((33, 10, 784, 64, 0), "relu"): 40}      # (case, activation)
MIN_DISTINCT = 60
ACTIVATIONS = (None, "relu")
PLANT_SHAPE = (70, 130, 200, 64, 128)


def act(y, activation):
    """LQ_ACT_NONE leaves v as it is; LQ_ACT_RELU is v > 0 ? v : (v != v ? v : +0)."""
    y = np.asarray(y, np.float32)
    if activation is None:
        return y
    assert activation == "relu"
    return np.where(y > 0, y, np.where(np.isnan(y), y, np.float32(0.0))).astype(np.float32)


def case(key):
    """(a, b, bias) of a case of the table."""
    return R.gemm_case(*key)


def reference(a, b, bias, activation):
    """The operand (dict) the fused call must write."""
    return R.operand_of_activation(act(R.gemm_reference(a, b, bias), activation), OUT_BLOCK)


def reference_buffers(a, b, bias, activation):
    return R.pack_layout(reference(a, b, bias, activation))


def scale_pattern(scales):
    """int8 [M][nbs]: 2 where the scale is NaN, 1 where it is 2^-126, 0 otherwise."""
    s = np.asarray(scales, np.float32)
    return np.where(np.isnan(s), 2, np.where(s == MIN_SCALE, 1, 0)).astype(np.int8)


def planted(name):
    """(a, b, bias, activation, want) of a planted case on PLANT_SHAPE (N = 130: output blocks of 64, 64 and 2 columns); ``want`` is
    the scale pattern claimed, int8 [70][3] as ``scale_pattern`` writes it: the pattern of the case before the plant (under relu a
    dozen rows have nothing positive in the two columns of block 2) with the planted pairs changed."""
    a, b, bias = case(PLANT_SHAPE)              # fresh arrays on every call
    activation = None if name == "huge_negative_bias" else "relu"
    if name == "zero_row":
        bias = None
    want = scale_pattern(reference(a, b, bias, activation)["scales"])
    assert not (want == 2).any()
    if name == "relu_empties_a_block":          # columns 64 .. 127 of every row are far below zero: block 1 is all +0 under relu
        bias[64:128] = np.float32(-1e30)
        want[:, 1] = 1
    elif name == "nan_scale_in_a":              # one scale block of line 5 of A: row 5 of Y is NaN, every block of it, no other row
        a["scales"][5, 1] = np.nan
        want[5, :] = 2
    elif name == "nan_scale_in_b":              # line 70 of B: column 70 of Y is NaN, block 1 of every row
        b["scales"][70, 0] = np.nan
        want[:, 1] = 2
    elif name == "inf_bias":                    # +Inf in column 3: block 0 of every row gets a NaN scale
        bias[3] = np.inf
        want[:, 0] = 2
    elif name == "huge_negative_bias":          # no activation: -1e30 in column 129 sets the scale of block 2, a finite one
        bias[129] = np.float32(-1e30)
    elif name == "zero_row":                    # a zero row of A without a bias: a zero row of Y, scale 2^-126 in every block
        a["codes"][7, :] = 0
        want[7, :] = 1
    else:
        raise KeyError(name)
    return a, b, bias, activation, want


PLANTED = ["relu_empties_a_block", "nan_scale_in_a", "nan_scale_in_b", "inf_bias", "huge_negative_bias", "zero_row"]
