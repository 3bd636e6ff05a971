"""CPU tests of ops.im2col_runs, the one rule by which ``call_mx`` and ``call_i8`` of a conv layer cut a batch into runs of whole
images: each run's im2col operand fits the C surface (lines * K < 2^31), its product fits either GEMM's grid (65535 * 64 lines)
and it holds at most ``max_lines`` lines -- unless one image alone is beyond a limit, which is then a run of its own.  Pure
arithmetic: no device, no library."""
import itertools

import pytest

from learned_quantization_amd import ops

GRID = 65535 * 64


def _check(B, per, K, max_lines):
    runs = ops.im2col_runs(B, per, K, max_lines)
    # a partition of range(B), in order, by non-empty runs
    assert runs[0][0] == 0 and runs[-1][1] == B
    assert all(b0 < b1 for b0, b1 in runs) and all(a[1] == b[0] for a, b in zip(runs, runs[1:]))
    limit = min(((1 << 31) - 1) // K, GRID, max_lines if max_lines is not None else GRID)
    for b0, b1 in runs:
        lines = (b1 - b0) * per
        if per > limit:                                    # one image is beyond a limit: exactly one image per run
            assert b1 - b0 == 1
        else:
            assert lines * K < 1 << 31 and lines <= GRID and (max_lines is None or lines <= max_lines)
    if per <= limit:                                       # and no run but the last could have taken another image
        assert all((b1 - b0 + 1) * per > limit for b0, b1 in runs[:-1])
    return runs


@pytest.mark.parametrize("K", [1, 27, 245, 4608, 1 << 20])
def test_runs_partition_the_batch_within_every_limit(K):
    for B, per in itertools.product([1, 2, 3, 7, 128], [1, 4, 25, 50176, GRID, GRID + 1]):
        for max_lines in (None, 1, per - 1, per, per + 1, 2 * per, 3 * per - 1, GRID, 1 << 40):
            if max_lines is None or max_lines >= 1:
                _check(B, per, K, max_lines)


def test_runs_of_the_cuts_the_device_tests_make():
    """tests/test_gpu_mx_conv.py::test_call_mx_is_the_composition and its int8 twin: B = 3, K = 5 * 7 * 7 = 245, OH * OW = 25 under
    'same' and 4 under 'valid', with max_lines None, OH * OW and 2 * OH * OW.  The runs are what both layers' own arithmetic gave
    before the rule was shared: images = max(1, min(B, fit // (OH * OW))) with fit = min(8765239, [4194240,] max_lines)."""
    for per in (25, 4):
        assert ops.im2col_runs(3, per, 245, None) == [(0, 3)]
        assert ops.im2col_runs(3, per, 245, per) == [(0, 1), (1, 2), (2, 3)]
        assert ops.im2col_runs(3, per, 245, 2 * per) == [(0, 2), (2, 3)]


def test_a_stem_batch_is_cut_at_the_grid_of_the_gemm():
    """128 images of 224 x 224 under a 3 x 3 'same' kernel on 3 channels: M = 6 422 528 lines, K = 27, so M * K < 2^31 and only the
    GEMM's grid cuts: 83 = 4194240 // 50176 images (4 164 608 lines), then the other 45."""
    assert ops.im2col_runs(128, 224 * 224, 27) == [(0, 83), (83, 128)]
    assert 128 * 224 * 224 * 27 < 1 << 31 and 83 * 50176 == 4164608 <= GRID < 84 * 50176


def test_one_image_beyond_a_limit_is_a_run_of_its_own():
    assert ops.im2col_runs(3, GRID + 1, 1) == [(0, 1), (1, 2), (2, 3)]
    assert ops.im2col_runs(2, 100, 1 << 30) == [(0, 1), (1, 2)]          # 100 lines * 2^30 is beyond 2^31: left to the C surface
    assert ops.im2col_runs(2, 100, 8, max_lines=99) == [(0, 1), (1, 2)]
