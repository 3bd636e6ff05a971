"""NumPy reference of the int8 im2col operand of a convolution (include/lq_hip.h: lq_i8_operand_im2col) and the geometries and data
sets of tests/test_gpu_i8_conv.py, so that tests/test_i8_conv_cpu.py can assert their conditions without a device.

Nothing is restated: the matrix is tests/_mx_conv_reference.py's ``im2col`` (written from the index definition of the header), the
operand tests/_i8_reference.py's ``operand_of_activation`` and the bytes its ``pack_layout``.

Geometries (B, C, H, W; KH x KW; stride; padding).  The first seven are the MX conv tests' (K = 27, 245, 576, 360, 160, 18, 36;
M = 50 .. 245), each with block 0, 64 and 128.  What the int8 kernel adds:
  (1,128,4,4; 3x3; 1; SAME)        K = 1152, M = 16: a long row at block 0 -- 72 units over four slices, 18 each, past the 4 a slice
                                   keeps in registers --; with block 128 nine full blocks
  (6,4,7,7; 3x3; 1; SAME)          M = 294: several thread-block chunks of lines (two of 256 lines, the plain form), M no multiple of 16
  (2,80,4,4; 1x1; 1; (2,0,2,0))    explicit padding with a 1 x 1 kernel: windows wholly in the padding, scale 2^-126 and codes 0;
                                   K = 80 puts them into the split form (block 0 and 128) and into the plain one (block 64)
The launch rule has one threshold: a span of up to 4 units of 16 k (one K step) takes the plain form, a longer one the split form.
Both sides: K = 27, 18, 36 and every block of 64 are 4 units; K = 80 (5 units read, 8 written), K = 160 and every block of 128 are
the shortest split spans.  The split form runs several chunks of 64 lines at M = 245 and 294 with block 128 and at K = 80, 160.
The kernel has a register cache (kI8ConvCache = 4 units per thread: the whole span of the plain form, 256 k over the four slices of
the split form): K = 360, 576 and 1152 at block 0 pass it, K = 245 and below do not."""
import numpy as np

import _i8_reference as I
import _mx_conv_reference as C
from _bounds import stable_seed

Geom = C.Geom
BLOCKS = (0, 64, 128)
LONG_ROW = Geom(1, 128, 4, 4, 3, 3, 1, 1, "SAME")
CHUNKED = Geom(6, 4, 7, 7, 3, 3, 1, 1, "SAME")
PADDING_ONLY = Geom(2, 80, 4, 4, 1, 1, 1, 1, (2, 0, 2, 0))
GEOMS = list(C.GEOMS) + [LONG_ROW, CHUNKED, PADDING_ONLY]
CASES = [(g, b) for g in GEOMS for b in BLOCKS]
STRIDED_GEOMS = C.STRIDED_GEOMS
EXACT_GEOMS = C.EXACT_GEOMS
MIN_SCALE = np.float32(2.0 ** -126)
MARGIN = np.float32(1.0 + 2.0 ** -22)                       # LQ_INIT_ABSMAX: s = absmax / 127 * (1 + 2^-22)


def case_id(case):
    g, block = case
    return f"{C.geom_id(g)}-b{block}"


def gaussian_input(g, seed=0):
    return C.gaussian_input(g, seed)


def reference(x, g, block):
    """(operand dict, documented code buffer, documented scale buffer) of input x (B, C, H, W)."""
    op = I.operand_of_activation(C.im2col(np.asarray(x, np.float32), g), block)
    return (op, *I.pack_layout(op))


def span_of(g, block):
    return block if block else C.dims(g)[1]


def windows_covering(g, block, b, c, h, w):
    """Boolean (M, nbs): the (line, scale block) pairs whose taps include pixel (b, c, h, w) -- tests/_mx_conv_reference.py's
    windows_covering generalised from blocks of 32 to a span: ``block``, or K when ``block`` is 0."""
    marker = np.zeros((g.B, g.C, g.H, g.W), np.float32)
    marker[b, c, h, w] = 1.0
    A = C.im2col(marker, g)
    span = span_of(g, block)
    nbs = -(-A.shape[1] // span)
    padded = np.zeros((A.shape[0], nbs * span), np.float32)
    padded[:, :A.shape[1]] = A
    return padded.reshape(A.shape[0], nbs, span).any(axis=2)


def live_pairs(g, block):
    """Boolean (M, nbs): the pairs that hold at least one pixel of the image."""
    A = C.im2col(np.ones((g.B, g.C, g.H, g.W), np.float32), g)
    span = span_of(g, block)
    nbs = -(-A.shape[1] // span)
    padded = np.zeros((A.shape[0], nbs * span), np.float32)
    padded[:, :A.shape[1]] = A
    return padded.reshape(A.shape[0], nbs, span).any(axis=2)


def planted_input(g, zero_channels, seed=1):
    """(x, nan_at, inf_at, big_at): Gaussian with all-zero channels, one NaN, one -Inf and one -1e30 pixel, in three corners: on
    the geometries of PLANTED no window holds two of them."""
    x = C.gaussian_input(g, seed=seed)
    nan_at, inf_at, big_at = (0, 0, g.H - 1, g.W - 1), (g.B - 1, g.C - 1, g.H - 1, 0), (g.B - 1, g.C - 2, 0, g.W - 1)
    x[:, zero_channels] = 0.0
    x[nan_at], x[inf_at], x[big_at] = np.nan, -np.inf, np.float32(-1e30)
    return x, nan_at, inf_at, big_at


# the zero channels are k = 49 .. 146 of K = 245 (the block 64 .. 127 of 64) and k = 126 .. 269 of K = 576 (128 .. 255: blocks of 64 and of 128)
PLANTED = [(C.GEOMS[1], (1, 2)), (C.GEOMS[2], tuple(range(14, 30)))]


def exact_input(g, seed=0):
    """x (B, C, H, W): integers in [-127, 127], channel 0 a plane of +-127.  Every SAME / VALID window holds a real pixel of every
    channel, so every im2col row has absmax exactly 127: its scale is 1 + 2^-22 and its codes are the pixels themselves."""
    rng = np.random.default_rng(stable_seed("i8-conv-exact-x", tuple(g), seed))
    x = rng.integers(-127, 128, size=(g.B, g.C, g.H, g.W)).astype(np.float32)
    x[:, 0] = np.where(rng.integers(0, 2, size=(g.B, g.H, g.W)) > 0, 127.0, -127.0)
    return x


def exact_kernel(g, co, seed=0):
    """(kernel HWIO (KH, KW, C, co) float32, bias (co,), scale, bias scale): integers over the whole byte times a power-of-two
    scalar scale -- the kernel is on its own 8-bit grid."""
    rng = np.random.default_rng(stable_seed("i8-conv-exact-w", tuple(g), co, seed))
    scale, bscale = np.float32(2.0 ** -7), np.float32(2.0 ** -6)
    k = (rng.integers(-128, 128, size=(g.KH, g.KW, g.C, co)) * scale).astype(np.float32)
    return k, (rng.integers(-128, 128, size=co) * bscale).astype(np.float32), scale, bscale
