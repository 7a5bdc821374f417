"""numpy definition of adaisp_raw_correct (include/adaisp.h): the integer defect rule on the uncorrected samples, then
the fp32 operations one at a time in the stated order (every intermediate an np.float32 array, so every operation rounds
once), np.rint (ties to even) and the clip. `correct` defines the output bit for bit; `exact` evaluates the same formula
in float64 without intermediate rounding (the fp32 inputs: steps, tables, black levels and scales, taken as they are),
against which tests/test_rawfix_host.py bounds it."""
import numpy as np

F = np.float32


def neighbours(plane):
    """int64 [8, H, W]: the same-position neighbours at (y +- 2 or y, x +- 2 or x), centre excluded, mirrored without
    edge repeat (np.pad 'reflect', period 2n - 2; a side of 2 folds twice, which np.pad does too)."""
    H, W = plane.shape
    p = np.pad(plane.astype(np.int64), 2, mode="reflect")
    return np.stack([p[2 + dy:2 + dy + H, 2 + dx:2 + dx + W] for dy in (-2, 0, 2) for dx in (-2, 0, 2) if dy or dx])


def defects(plane, dpc):
    """The plane after the defect rule, as int64. dpc < 0 (or None): unchanged."""
    v = plane.astype(np.int64)
    if dpc is None or dpc < 0:
        return v
    n = neighbours(plane)
    hi, lo = n.max(0), n.min(0)
    hot = v > hi + dpc
    dead = ~hot & (v + dpc < lo)
    return np.where(hot, hi, np.where(dead, lo, v))


def steps(shape, grid_shape):
    """(step_y, step_x) as the host computes them: (grid - 1) / (side - 1) in float64, one cast to fp32."""
    (H, W), (gh, gw) = shape, grid_shape
    return F((gh - 1) / (H - 1)), F((gw - 1) / (W - 1))


def _axis(n, step, g, dtype):
    f = (np.arange(n).astype(F) * F(step)).astype(F)                 # (float)y * step: one fp32 multiply
    i = np.minimum(np.clip(f, 0, 2147483520.0).astype(np.int64), g - 2)
    if dtype is F:
        return i, (f - i.astype(F)).astype(F)
    # the cell is the fp32 one in both evaluations (a decision, not a rounding; the interpolant is continuous across cells)
    return i, np.arange(n) * np.float64(F(step)) - i


def _position(H, W):
    yy, xx = np.mgrid[0:H, 0:W]
    return 2 * (yy & 1) + (xx & 1)


def gain(shape, table, step_y, step_x, dtype=F):
    """[H, W] of g for a [4, gh, gw] fp32 table; dtype F: one fp32 operation at a time; np.float64: no rounding."""
    H, W = shape
    table = np.asarray(table, F)
    _, gh, gw = table.shape
    iy, ty = _axis(H, step_y, gh, dtype)
    ix, tx = _axis(W, step_x, gw, dtype)
    k = _position(H, W)
    T = table.astype(dtype)
    IY, IX = iy[:, None], ix[None, :]
    TY, TX = ty[:, None].astype(dtype), tx[None, :].astype(dtype)
    t00, t01, t10, t11 = T[k, IY, IX], T[k, IY, IX + 1], T[k, IY + 1, IX], T[k, IY + 1, IX + 1]
    if dtype is F:
        a = (t00 + (TX * (t01 - t00).astype(F)).astype(F)).astype(F)
        b = (t10 + (TX * (t11 - t10).astype(F)).astype(F)).astype(F)
        return (a + (TY * (b - a).astype(F)).astype(F)).astype(F)
    a = t00 + TX * (t01 - t00)
    b = t10 + TX * (t11 - t10)
    return a + TY * (b - a)


def _value(plane, black, scale, black_out, dpc, table, step, dtype):
    H, W = plane.shape
    k = _position(H, W)
    v = defects(plane, dpc).astype(dtype)
    bk, sk = np.asarray(black, F).astype(dtype)[k], np.asarray(scale, F).astype(dtype)[k]
    if table is None:
        g = np.ones((H, W), dtype)
    else:
        sy, sx = steps(plane.shape, np.shape(table)[1:]) if step is None else step
        g = gain(plane.shape, table, sy, sx, dtype)
    if dtype is F:
        u = ((v - bk).astype(F) * g).astype(F)
        return ((u * sk).astype(F) + F(black_out)).astype(F)
    return (v - bk) * g * sk + np.float64(F(black_out))


def correct(plane, black=(0, 0, 0, 0), scale=(1, 1, 1, 1), black_out=0.0, dpc=-1, table=None, step=None):
    """One image of adaisp_raw_correct: uint16 [H, W]. black, scale: four numbers by position (taken as fp32); table: None
    (grid < 0) or fp32 [4, gh, gw]; step: (step_y, step_x), default `steps`; dpc < 0 or None: no defect rule."""
    with np.errstate(invalid="ignore", over="ignore"):
        u = _value(plane, black, scale, black_out, dpc, table, step, F)
        r = np.rint(u)
        r = np.where(np.isnan(r), 0, r)
        return np.clip(r, 0, 65535).astype(np.uint16)


def exact(plane, black=(0, 0, 0, 0), scale=(1, 1, 1, 1), black_out=0.0, dpc=-1, table=None, step=None):
    """float64 [H, W]: u of the same formula before the rounding and the clip, without intermediate rounding."""
    return _value(plane, black, scale, black_out, dpc, table, step, np.float64)


def scales(black, white_in, black_out, white_out):
    """The host's scale[k] = (white_out - black_out) / (white_in - black[k]): float64, one cast to fp32."""
    return ((float(white_out) - float(black_out)) / (float(white_in) - np.asarray(black, np.float64))).astype(F)


def table(gh, gw, seed=0, depth=0.6):
    """A seeded fp32 [4, gh, gw] gain table: 1 at the centre rising towards the corners, a little different per position."""
    rs = np.random.RandomState(seed)
    yy, xx = np.mgrid[0:gh, 0:gw].astype(np.float64)
    r2 = ((yy / (gh - 1) - 0.5) ** 2 + (xx / (gw - 1) - 0.5) ** 2) * 2.0
    return np.stack([1.0 + depth * (1.0 + 0.1 * k) * r2 + rs.uniform(0, 0.02, (gh, gw)) for k in range(4)]).astype(F)


def plane(h, w, seed, black=64, white=4095, hot=0.01):
    """A seeded uint16 [h, w] plane: smooth content with noise inside black .. white and a share `hot` of hot / dead
    samples."""
    rs = np.random.RandomState(seed)
    yy, xx = np.mgrid[0:h, 0:w].astype(np.float64)
    v = 0.5 + 0.4 * np.sin(0.07 * xx + 0.05 * yy + seed) + rs.normal(0, 0.03, (h, w))
    p = np.clip(np.rint(black + np.clip(v, 0, 1) * (white - black)), 0, 65535).astype(np.uint16)
    bad = rs.uniform(size=(h, w)) < hot
    p[bad] = np.where(rs.uniform(size=int(bad.sum())) < 0.5, white, 0).astype(np.uint16)
    return p


# ------------------------------------------------------------------------------------------------------------ hand-placed
def _base(h=10, w=12):
    """1000 + 10 k at every sample of position k: every same-position neighbourhood is flat."""
    yy, xx = np.mgrid[0:h, 0:w]
    return (1000 + 10 * (2 * (yy & 1) + (xx & 1))).astype(np.uint16)


# every position at a corner, on an edge and in the interior of a 10 x 12 plane; no two of one position within reach
SITES = [(0, 0), (0, 11), (9, 0), (9, 11), (0, 6), (0, 5), (9, 6), (9, 5), (4, 8), (4, 9), (5, 8), (5, 9)]


def defect_cases():
    """[(plane, dpc, the corrected plane written down by hand)]."""
    base, cases = _base(), []
    hot, dead = base.copy(), base.copy()
    for y, x in SITES:
        hot[y, x] += 2000
        dead[y, x] = 0
    cases.append((hot, 50, base))                                     # isolated hot samples -> their neighbours' maximum
    cases.append((dead, 50, base))                                    # isolated dead samples -> their neighbours' minimum
    edge = base.copy()
    edge[4, 4] += 50                                                  # exactly dpc above the maximum: stays
    edge[6, 8] += 51                                                  # one more: corrected
    edge[5, 3] -= 50                                                  # exactly dpc below the minimum: stays
    edge[7, 7] -= 51
    want = edge.copy()
    want[6, 8], want[7, 7] = base[6, 8], base[7, 7]
    cases.append((edge, 50, want))
    pair = base.copy()
    pair[4, 4] = pair[4, 6] = 3000                                    # each sees the other uncorrected: both stay
    pair[3, 1] = pair[5, 1] = 0
    pair[1, 8] = 3000                                                 # row 1 mirrors onto itself (-1 -> 1): its own neighbour
    cases.append((pair, 50, pair.copy()))
    zero = base.copy()
    zero[2, 2] += 1                                                   # dpc = 0: anything above the maximum is clamped
    zero[2, 7] -= 1
    cases.append((zero, 0, base))
    cases.append((hot, -1, hot.copy()))                               # dpc < 0: nothing changes
    return cases


def tie_case():
    """(plane, options, result): gain 0.5 on odd values: n + 0.5 goes to the even one of n, n + 1."""
    n = np.arange(24).reshape(4, 6)
    return (2 * n + 1).astype(np.uint16), dict(scale=(0.5,) * 4), (n + (n & 1)).astype(np.uint16)


def clip_case():
    """(plane, options, result): (v - 1000) * 4 leaves [0, 65535] on both sides."""
    p = np.array([[0, 999, 1000, 1001], [2000, 17383, 17384, 65535]], np.uint16)
    want = np.array([[0, 0, 0, 4], [4000, 65532, 65535, 65535]], np.uint16)
    return p, dict(black=(1000.0,) * 4, scale=(4.0,) * 4), want
