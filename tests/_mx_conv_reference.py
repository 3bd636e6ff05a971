"""NumPy reference of the im2col operand of a convolution (include/lq_hip.h: lq_mx_im2col_dims / lq_mx_operand_im2col) and the
geometries and data sets of tests/test_gpu_mx_conv.py, so that tests/test_mx_conv_cpu.py can assert their conditions without a device.

``im2col`` is written from the index definition of the header -- line m = (b OH + oh) OW + ow, reduction index k = (c KH + i) KW + j,
A[m][k] = X[b][c][oh stride_h - pad_top + i][ow stride_w - pad_left + j] or +0 -- not from F.unfold; the CPU file holds it against
F.unfold and against F.conv2d.  The bytes of the operand are tests/_mx_gemm_reference.py's: operand_of_activation(A) and pack_layout."""
from collections import namedtuple

import numpy as np

import _mx_gemm_reference as G
from _bounds import stable_seed

# padding: "SAME" (TensorFlow's, asymmetric where it is), "VALID", or an explicit (top, bottom, left, right)
Geom = namedtuple("Geom", "B C H W KH KW sh sw padding")

# what each exercises: tests/test_gpu_mx_conv.py's docstring
GEOMS = [
    Geom(2, 3, 5, 5, 3, 3, 1, 1, "SAME"),
    Geom(2, 5, 9, 10, 7, 7, 2, 2, "SAME"),
    Geom(1, 64, 4, 4, 3, 3, 1, 1, "SAME"),
    Geom(3, 40, 6, 6, 3, 3, 1, 1, "VALID"),
    Geom(2, 160, 5, 5, 1, 1, 2, 2, "SAME"),
    Geom(2, 6, 6, 8, 1, 3, 2, 1, "SAME"),
    Geom(5, 4, 7, 7, 3, 3, 1, 1, "SAME"),
]
STRIDED_GEOMS = GEOMS[:3]
EXACT_GEOMS = [GEOMS[1], GEOMS[2]]      # K = 245 and K = 576
METHODS = ("mx", "cover")


def geom_id(g):
    pad = g.padding.lower() if isinstance(g.padding, str) else "p" + ".".join(map(str, g.padding))
    return f"{g.B}x{g.C}x{g.H}x{g.W}-k{g.KH}x{g.KW}-s{g.sh}x{g.sw}-{pad}"


def same_padding(size, k, s):
    """TensorFlow 'SAME', restated: out = ceil(size / s), total = max((out - 1) s + k - size, 0), the odd pixel goes after."""
    out = -(-size // s)
    total = max((out - 1) * s + k - size, 0)
    return total // 2, total - total // 2


def padding_of(g):
    """(top, bottom, left, right)."""
    if not isinstance(g.padding, str):
        top, bottom, left, right = (int(p) for p in g.padding)
        return (top, bottom, left, right)
    if g.padding == "VALID":
        return (0, 0, 0, 0)
    return (*same_padding(g.H, g.KH, g.sh), *same_padding(g.W, g.KW, g.sw))


def dims(g):
    """(M, K, OH, OW) from the header's formulas."""
    top, bottom, left, right = padding_of(g)
    OH, OW = (g.H + top + bottom - g.KH) // g.sh + 1, (g.W + left + right - g.KW) // g.sw + 1
    return g.B * OH * OW, g.C * g.KH * g.KW, OH, OW


def im2col(x, g):
    """A (M, K) of x (B, C, H, W), in x's dtype, from the index definition."""
    top, _, left, _ = padding_of(g)
    M, K, OH, OW = dims(g)
    A = np.zeros((g.B, OH, OW, g.C, g.KH, g.KW), x.dtype)
    for i in range(g.KH):
        for j in range(g.KW):
            ih, iw = np.arange(OH) * g.sh - top + i, np.arange(OW) * g.sw - left + j
            vh, vw = np.flatnonzero((ih >= 0) & (ih < g.H)), np.flatnonzero((iw >= 0) & (iw < g.W))
            if vh.size and vw.size:
                A[np.ix_(np.arange(g.B), vh, vw, np.arange(g.C), [i], [j])] = \
                    x[np.ix_(np.arange(g.B), np.arange(g.C), ih[vh], iw[vw])].transpose(0, 2, 3, 1)[..., None, None]
    return A.reshape(M, K)


def windows_covering(g, b, c, h, w):
    """Boolean (M, ceil(K / 32)): the blocks whose 32 taps include pixel (b, c, h, w) -- counted from the definition, tap by tap."""
    marker = np.zeros((g.B, g.C, g.H, g.W), np.float32)
    marker[b, c, h, w] = 1.0
    A = im2col(marker, g)
    nb = -(-A.shape[1] // G.BLOCK)
    padded = np.zeros((A.shape[0], nb * G.BLOCK), np.float32)
    padded[:, :A.shape[1]] = A
    return padded.reshape(A.shape[0], nb, G.BLOCK).any(axis=2)


def gaussian_input(g, seed=0):
    """x (B, C, H, W): Gaussian, every (image, channel) plane at a magnitude of its own (2^-6 .. 2^6)."""
    rng = np.random.default_rng(stable_seed("mx-conv-x", tuple(g), seed))
    return (rng.standard_normal((g.B, g.C, g.H, g.W)) * np.exp2(rng.integers(-6, 7, size=(g.B, g.C, 1, 1)))).astype(np.float32)


def plain_gaussian_input(g, seed=0):
    """x (B, C, H, W): standard normal, one magnitude throughout -- the data the yardstick of the GEMM's error was measured on
    (tests/_mx_gemm_reference.py, random_case)."""
    rng = np.random.default_rng(stable_seed("mx-conv-plain-x", tuple(g), seed))
    return rng.standard_normal((g.B, g.C, g.H, g.W)).astype(np.float32)


def exact_input(g, seed=0):
    """x (B, C, H, W) drawn from G.EXACT_VALUES: on the grid of every format under the scale either rule takes from its block."""
    rng = np.random.default_rng(stable_seed("mx-conv-exact-x", tuple(g), seed))
    return G.EXACT_VALUES[rng.integers(0, G.EXACT_VALUES.size, size=(g.B, g.C, g.H, g.W))]


def exact_kernel(g, co, seed=0):
    """(kernel HWIO (KH, KW, C, co), bias (co,)) drawn from G.EXACT_VALUES, for layers whose scales are all 1 (byte 127)."""
    rng = np.random.default_rng(stable_seed("mx-conv-exact-w", tuple(g), co, seed))
    k = G.EXACT_VALUES[rng.integers(0, G.EXACT_VALUES.size, size=(g.KH, g.KW, g.C, co))]
    return k, G.EXACT_VALUES[rng.integers(0, G.EXACT_VALUES.size, size=co)]


def kernel_matrix(k_hwio):
    """(co, K): the kernel's lines over k = (c KH + i) KW + j, the memory order of OIHW."""
    return np.ascontiguousarray(k_hwio.transpose(3, 2, 0, 1)).reshape(k_hwio.shape[3], -1)
