"""The launch rule of the group-wise kernels restated in Python, and the case table that reaches every run-time branch of it.

``launch_shape`` restates group_launch and group_vec_ok of csrc/lq_kernels.hip (the single-tensor launchers and fill_group_task
all ask group_launch; fill_group_task passes the group extent nb instead of min(nb, 32768) as max_groups_y -- the two agree
wherever the row split can exceed 1, see ``launch_shape``).  It exists ONLY so that tests/test_group_forms_cpu.py can prove that
``FORMS`` (with AXIS0 / AXIS1 of tests/test_gpu_groupwise.py) takes every branch; profiles/group_forms/kernel_coverage.txt holds
the kernel names and grids of a traced run next to what it predicts.  It is never used to compute an expected output: those come
from tests/_group_reference.py alone.

The second half builds the inputs of the data-driven tests (edge quotients, scales outside the fast-division window, random
geometry), so that the CPU file can assert their conditions on the reference without a device."""
import numpy as np

from _bounds import stable_seed
from _group_reference import expand_scale, make_case, scale_shape

K_BLOCK = 256                 # threads of a block (csrc/lq_common.hpp: kBlock)
COLS_LANES4, COLS_LANES1 = 16, 64
MAX_GRID_Y = 32768
BLOCK_CAP = 2048              # the forward splits the rows of a group only while tiles * groups * nz stays below it
TEAMS = (1, 2, 4, 8, 16, 32, 64)


def launch_shape(R, C, axis, gs, aligned16=True):
    """What the host picks for a tensor [R][C] with groups of ``gs`` along ``axis``; ``aligned16``: every dense base on the
    16-byte grid.  Keys: form (cols4 | cols1 | rows4 | rows1), gs (clamped), nb, last (length of the last group of a line), and

      column forms  tiles (grid.x), grid_y, trips (most trips of the group loop any block takes), second_trip (blocks along y that
                    take a second trip), nz (forward row split, grid.z), nz_by_gs (what gs alone would allow), capped (nz < nz_by_gs:
                    the 2048-block cap decided), blocks_fwd, blocks_bwd, dead (lanes of the last column tile without a column)
      row forms     team (lanes per (row, group) pair), pairs, per_block, blocks, dead (teams of the last block without a pair)"""
    length = R if axis == 0 else C
    gs = min(int(gs), length)
    nb = -(-length // gs)
    vec = bool(aligned16) and C % 4 == 0 and (axis == 0 or gs % 4 == 0)
    d = dict(gs=gs, nb=nb, last=length - (nb - 1) * gs)
    if axis == 0:
        lanes = COLS_LANES4 if vec else COLS_LANES1
        slots = K_BLOCK // lanes
        tiles = -(-C // 64)                                   # 16 lanes x float4 or 64 scalar lanes: 64 columns either way
        grid_y = min(nb, MAX_GRID_Y)

        def split(cap):
            nz = 1
            while nz < 4 and (not cap or tiles * grid_y * nz < BLOCK_CAP) and slots * nz * 4 <= gs:
                nz *= 2
            return nz
        nz, nz_by_gs = split(True), split(False)
        # the batch asks with nb in place of grid_y: they differ only above 32768 groups, where both are past the cap
        assert grid_y == nb or tiles * grid_y >= BLOCK_CAP
        columns_of_a_tile = lanes * (4 if vec else 1)
        d.update(form="cols4" if vec else "cols1", tiles=tiles, grid_y=grid_y, trips=-(-nb // grid_y), second_trip=nb - grid_y,
                 nz=nz, nz_by_gs=nz_by_gs, capped=nz < nz_by_gs, blocks_fwd=tiles * grid_y * nz, blocks_bwd=tiles * grid_y,
                 dead=(tiles * columns_of_a_tile - C) // (4 if vec else 1))
    else:
        items = (gs + 3) // 4 if vec else gs
        log_team = 0
        while log_team < 6 and (4 << log_team) < items:
            log_team += 1
        pairs, per_block = R * nb, K_BLOCK >> log_team
        blocks = -(-pairs // per_block)
        d.update(form="rows4" if vec else "rows1", team=1 << log_team, pairs=pairs, per_block=per_block, blocks=blocks,
                 dead=blocks * per_block - pairs)
    return d


# (R, C, axis, gs), what the case is there for, and the extra variants tests/test_gpu_group_forms.py::test_forms runs it in
FORMS = [
    ((9, 200, 1, 64), "rows4, team 4, last group 8", ()),
    ((5, 1100, 1, 256), "rows4, team 16, 2 blocks, last group 76", ("nearest", "unsigned")),
    ((3, 2600, 1, 1024), "rows4, team 64, last group 552", ("nearest",)),
    ((3, 2068, 1, 516), "rows4, team 64, last group of one float4", ("nearest",)),
    ((70, 12, 1, 3), "rows1 (gs % 4 != 0 on a 4-divisible C), team 1", ()),
    ((11, 203, 1, 30), "rows1, team 8", ()),
    ((7, 333, 1, 50), "rows1, team 16", ("nearest", "unsigned")),
    ((6, 515, 1, 127), "rows1, team 32", ()),
    ((3, 1001, 1, 333), "rows1, team 64, last group 2", ("nearest",)),
    # three widths the lists of tests/test_gpu_groupwise.py do not hold either (the group batch's set and a layer test launch them)
    ((6, 68, 1, 24), "rows4, team 2, last group 20", ()),
    ((3, 1300, 1, 400), "rows4, team 32, last group 100", ()),
    ((13, 45, 1, 10), "rows1, team 4, last group 5", ()),
    ((40000, 4, 0, 1), "cols4, nb = 40000 > 32768: second trip for 7232 blocks", ("nearest",)),
    ((33000, 3, 0, 1), "cols1, second trip", ("nearest", "unsigned")),
    ((70001, 4, 0, 2), "cols4, second trip, ragged last group of one row", ("nearest",)),
    ((50, 7, 0, 20), "cols1, nz = 2 by gs", ()),
    ((200, 64, 0, 64), "cols4, nz = 2 by gs, last group 8", ("unsigned",)),
    ((2240, 1030, 0, 32), "cols1, nz = 2 by the 2048-block cap (gs allows 4)", ()),
    ((2000, 1030, 0, 16), "cols1, nz = 1 by the cap (gs allows 2)", ()),
    ((4224, 2048, 0, 128), "cols4, nz = 2 by the cap; 8.6 M elements, the one large case", ()),
]
LARGE = (4224, 2048, 0, 128)
FORM_CASES = [f[0] for f in FORMS]
VARIANTS = {"floor": ((-8, 7), "floor"), "nearest": ((-8, 7), "nearest"), "unsigned": ((0, 15), "floor")}


def form_variants():
    """[(case, variant name)]: every case in floor [-8, 7]; the team-16 / team-64 / second-trip cases in nearest; four in [0, 15]."""
    return [(case, v) for case, _, extra in FORMS for v in ("floor",) + tuple(extra)]


# ------------------------------------------------------------------------------------------------------------ edge quotients
EDGE_RANGES = [(-8, 7), (0, 15), (-128, 127)]
EDGE_SHAPES = [(200, 64, 0, 64),        # cols4: fq_quot4c
               (96, 130, 0, 96),        # cols1: div_by_uniform on axis 0
               (5, 1100, 1, 256),       # rows4: fq_quot4
               (7, 333, 1, 50)]         # rows1: div_by_uniform on axis 1
CLIP_DESCRIPTORS = [(1, 5, 4100), (256, 16, 49), (64, 130, 4)]      # of tests/test_gpu_clip.py: a ROW, a COL with cut float4s, the inner-4 COL


def edge_scales(rng, shape):
    """2^U(-12, 3): random exponents AND random full mantissas -- the reciprocal is inexact for all but a power of two."""
    return np.exp2(rng.uniform(-12.0, 3.0, size=shape)).astype(np.float32)


def power_of_two_share(s):
    return float(np.mean((np.asarray(s, np.float32).view(np.uint32) & 0x7FFFFF) == 0))


def edge_data(sb, pos, qmin, qmax, rounding):
    """P on the element grid of ``sb`` (the scale of every element): element with sequence position ``pos`` holds member
    pos % 3 of triple (pos // 3) % (qmax - qmin + 5): c = fl32(m * s), the float below c, the float above c, with m = n (floor) or
    n + 1/2 (nearest) and n running over [qmin - 2, qmax + 2].  Returns (P, share): the share of the triples (by their c elements)
    whose two neighbours round to different integers under the reference's arithmetic (float32 division, floor / rint)."""
    sb = np.asarray(sb, np.float32)
    count = qmax - qmin + 5
    idx = np.asarray(pos, np.int64) % (3 * count)
    m = ((qmin - 2) + idx // 3).astype(np.float32) + np.float32(0.5 if rounding == "nearest" else 0.0)
    c = m * sb
    assert c.dtype == np.float32
    down, up = np.nextafter(c, np.float32(-np.inf)), np.nextafter(c, np.float32(np.inf))
    which = idx % 3
    P = np.where(which == 0, c, np.where(which == 1, down, up)).astype(np.float32)
    rnd = np.floor if rounding == "floor" else np.rint
    with np.errstate(all="ignore"):
        straddle = rnd(down / sb) != rnd(up / sb)
    return P, float(straddle[which == 0].mean())


def edge_group_case(seed, R, C, axis, gs, qmin, qmax, rounding):
    """(P, s, dy, share) of a group-wise tensor: every group starts at a random triple, then runs through the triples in order."""
    rng = np.random.default_rng(seed)
    shape = scale_shape(R, C, axis, gs)
    s = edge_scales(rng, shape)
    first = rng.integers(0, qmax - qmin + 5, size=shape).astype(np.float32)      # carried on the grid by the scale's index rule
    rot = expand_scale(first, R, C, axis, gs).astype(np.int64)
    along = (np.arange(R) % gs)[:, None] if axis == 0 else (np.arange(C) % gs)[None, :]
    P, share = edge_data(expand_scale(s, R, C, axis, gs), 3 * rot + along, qmin, qmax, rounding)
    return P, s, rng.standard_normal((R, C)).astype(np.float32), share


def edge_clip_case(seed, desc, qmin, qmax, rounding):
    """The same data on an (outer, G, inner) descriptor of the one-axis clipped op, s of shape (1, G, 1)."""
    outer, G, inner = desc
    rng = np.random.default_rng(seed)
    s = edge_scales(rng, (1, G, 1))
    first = rng.integers(0, qmax - qmin + 5, size=(1, G, 1))
    pos = 3 * first + np.arange(outer)[:, None, None] * inner + np.arange(inner)[None, None, :]
    P, share = edge_data(np.broadcast_to(s, desc), pos, qmin, qmax, rounding)
    return P, s, rng.standard_normal(desc).astype(np.float32), share


# ------------------------------------------------------------------------------------- scales outside the fast-division window
def _f32(bits):
    return np.array([bits], np.uint32).view(np.float32)[0]


_P40, _M40 = np.float32(2.0 ** 40), np.float32(2.0 ** -40)
BAD_SCALES = np.array([_M40, np.nextafter(_M40, np.float32(0)), _P40, np.nextafter(_P40, np.float32(np.inf)), _f32(0x3BFFFFFF),
                       -0.25, 0.0, -0.0, 1e-41, 3e38, np.inf, np.nan], np.float32)
_P81 = np.float32(2.0 ** 81)
SPECIAL_X = np.array([2.0 ** -81, 2.0 ** -80, _P81, np.nextafter(_P81, np.float32(0)), 0.0, -0.0, 1e-40, np.inf, -np.inf, np.nan],
                     np.float32)
WINDOW_SHAPES = [(200, 64, 0, 64), (96, 130, 0, 96), (9, 200, 1, 64), (11, 203, 1, 30)]      # cols4, cols1, rows4, rows1


def plant_specials(P, rng, rounds=6):
    """One member of chosen float4s (flat element index 4 f + lane) set to each of SPECIAL_X in turn, ``rounds`` times over (each
    round holds one NaN, which spoils ds of its group by definition); returns the positions."""
    flat = P.reshape(-1)
    quads = flat.size // 4
    picks = rng.choice(quads, size=min(quads, rounds * SPECIAL_X.size), replace=False)
    at = picks * 4 + rng.integers(0, 4, size=picks.size)
    flat[at] = SPECIAL_X[np.arange(picks.size) % SPECIAL_X.size]
    return at


def interleave_bad_scales(s, C, axis):
    """(s, bad): the scales ``s`` with the values of BAD_SCALES interleaved -- axis 0: exactly one of every four columns of a
    float4 (its lane moves with the group and the float4), axis 1: every other group of a row, shifted by the row.  ``bad``: bool,
    in the shape of s; every value of BAD_SCALES is reached."""
    a, b = np.indices(s.shape)
    if axis == 0:                      # s[g][c]
        bad = (b % 4) == ((a + b // 4) % 4)
        which = (a * (-(-C // 4)) + b // 4) % BAD_SCALES.size
    else:                              # s[r][g]
        bad = ((a + b) % 2) == 1
        which = ((a * s.shape[1] + b) // 2) % BAD_SCALES.size
    s = np.where(bad, BAD_SCALES[which], s).astype(np.float32)
    assert set(which[bad].tolist()) == set(range(BAD_SCALES.size)), "a scale value is not reached"
    return s, bad


def window_group_case(seed, R, C, axis, gs):
    """(P, s, dy, bad): ordinary inputs (make_case) with scales of BAD_SCALES interleaved (interleave_bad_scales) and special
    values planted in P.  ``bad``: bool, in the shape of s."""
    P, s, dy = make_case(seed, R, C, axis, gs)
    rng = np.random.default_rng(seed + 1)
    s, bad = interleave_bad_scales(s, C, axis)
    plant_specials(P, rng)
    return P, s, dy, bad


def window_clip_cases(seed, desc):
    """[(P, s, dy, bad)] on an (outer, G, inner) descriptor: every odd group holds a value of BAD_SCALES; as many passes as it takes
    to reach all of them.  P ~ N(0, 1) * 8 * 2^-7 with special values planted."""
    outer, G, inner = desc
    slots = G // 2
    cases = []
    for k in range(-(-BAD_SCALES.size // slots)):
        rng = np.random.default_rng(seed + k)
        s = np.exp2(rng.uniform(-9.0, -5.0, size=(1, G, 1))).astype(np.float32)
        g = np.arange(G)
        bad = (g % 2 == 1).reshape(1, G, 1)
        s = np.where(bad, BAD_SCALES[(k * slots + g // 2) % BAD_SCALES.size].reshape(1, G, 1), s).astype(np.float32)
        P = rng.standard_normal(desc).astype(np.float32) * np.float32(2.0 ** -4)
        plant_specials(P, rng, rounds=1)
        cases.append((P, s, rng.standard_normal(desc).astype(np.float32), bad))
    return cases


# ---------------------------------------------------------------------------------------------------------- random geometry
GEOMETRY_DRAWS = 64
GEOMETRY_RANGES = [(-8, 7), (0, 15), (-2, 1)]


def _extent(rng):
    if rng.random() < 0.75:            # multiples of 4 and their +-1 neighbours: where the float4 forms begin and end
        return int(np.clip(4 * rng.integers(1, 76) + rng.integers(-1, 2), 1, 300))
    return int(rng.integers(1, 301))


def random_geometry(i):
    """Draw i: dict(k, R, C, axis, gs, rounding, range, residue); ``k = stable_seed("geometry", i)`` seeds the draw and its data."""
    k = stable_seed("geometry", i)
    rng = np.random.default_rng(k)
    R, C = _extent(rng), _extent(rng)
    assert R * C <= 100000
    axis = int(rng.integers(0, 2))
    length = R if axis == 0 else C
    sizes = [1, 2, 3, 4, 5, 7, 8, 16, 31, 32, 64, 100, 128, max(length - 1, 1), length, length + 1, 2 * length]
    return dict(k=k, R=R, C=C, axis=axis, gs=int(sizes[rng.integers(0, len(sizes))]), rounding=("floor", "nearest")[int(rng.integers(0, 2))],
                range=GEOMETRY_RANGES[int(rng.integers(0, 3))], residue=int(4 * rng.integers(0, 4)))
