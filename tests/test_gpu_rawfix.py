"""adaisp_raw_correct on the MI355X (csrc/isp_raw_correct.hip): packed uint16 planes -> corrected uint16 planes in one
launch, against the numpy definition (tests/_rawfixref.py) bit for bit. `dst` is pre-filled with a sentinel between guard
bytes, so an unwritten sample, a write outside a plane and a write outside `dst` all show."""
import numpy as np
import pytest
import torch

import _rawfixref as X
from adaptiveisp_amd import _lib
from adaptiveisp_amd.rawcal import fill_rawfix

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SENT = 0xA5                                                           # every untouched byte of dst
GUARD = 256
# The kernel's tile is RF_ROWS x RF_COLS = 16 x 248 samples, its ring 2. 20 x 497: one sample wider than two tiles;
# 33 x 260: one row taller than two tiles (and one tile and 12 columns wide).
TILE_H, TILE_W = 16, 248
SHAPES = [(2, 2), (3, 5), (37, 53), (40, 64), (20, 2 * TILE_W + 1), (2 * TILE_H + 1, 260)]
BLACK = (60.0, 64.0, 66.5, 71.0)                                      # four distinct levels, one of them not whole
WHITE_IN, BLACK_OUT, WHITE_OUT = 4000.0, 64.0, 4095.0


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _run(planes, cfgs, offsets=None, dst_offsets=None, mutate=None, gain_cut=0):
    """One launch. cfgs: per plane a dict(black, scale, black_out, dpc, table). Returns (per-plane uint16 results or None
    where `dst` kept its sentinel over the whole plane, the records)."""
    pos, offs = 0, []
    for b, p in enumerate(planes):
        off = pos if offsets is None else offsets[b]
        offs.append(off)
        pos = (off + p.nbytes + 15) // 16 * 16
    doffs = offs if dst_offsets is None else dst_offsets
    nbytes = max(pos, max(o + p.nbytes for o, p in zip(doffs, planes))) + 16
    src = np.zeros(nbytes, np.uint8)
    rec = np.zeros(len(planes), _lib.RAWFIX_DESC)
    tabs, words = [], 0
    for b, (p, c) in enumerate(zip(planes, cfgs)):
        src[offs[b]:offs[b] + p.nbytes] = p.reshape(-1).view(np.uint8)
        t = c.get("table")
        fill_rawfix(rec[b], p.shape, offs[b], doffs[b], c.get("black", (0,) * 4), c.get("scale", (1,) * 4),
                    c.get("black_out", 0.0), c.get("dpc", -1), None if t is None else (words, t.shape[1], t.shape[2]))
        if t is not None:
            tabs.append(t.reshape(-1))
            words += t.size
    if mutate:
        mutate(rec)
    gains = _dev(np.concatenate(tabs).astype(np.float32)) if tabs else None
    if gains is not None and gain_cut:
        gains = gains[:-gain_cut]
    buf = torch.full((nbytes + 2 * GUARD,), SENT, dtype=torch.uint8, device=DEV)
    out = buf[GUARD:GUARD + nbytes]
    _lib.raw_correct(_dev(src), _dev(rec.view(np.uint8)), gains, out=out)
    torch.cuda.synchronize()
    host = buf.cpu().numpy()
    assert (host[:GUARD] == SENT).all() and (host[GUARD + nbytes:] == SENT).all()
    host = host[GUARD:GUARD + nbytes]
    got, keep = [], np.ones(nbytes, bool)
    for b, p in enumerate(planes):
        raw = host[doffs[b]:doffs[b] + p.nbytes]
        keep[doffs[b]:doffs[b] + p.nbytes] = False
        got.append(None if (raw == SENT).all() else raw.view(np.uint16).reshape(p.shape).copy())
    assert (host[keep] == SENT).all()                                 # nothing between or behind the planes
    return got, rec


def _want(p, c):
    return X.correct(p, c.get("black", (0,) * 4), c.get("scale", (1,) * 4), c.get("black_out", 0.0), c.get("dpc", -1),
                     c.get("table"))


def _cfg(dpc=40, grid=(5, 7), seed=0):
    return dict(black=BLACK, scale=X.scales(BLACK, WHITE_IN, BLACK_OUT, WHITE_OUT), black_out=BLACK_OUT, dpc=dpc,
                table=None if grid is None else X.table(grid[0], grid[1], seed))


# ------------------------------------------------------------------------------------------------------------ shapes
@pytest.mark.parametrize("grid", [(2, 2), (5, 7)])
@pytest.mark.parametrize("shape", SHAPES)
def test_shape_is_the_definition(shape, grid):
    H, W = shape
    rs = np.random.RandomState(1000 * H + W)
    smooth = X.plane(H, W, H + W, hot=0.02)
    noisy = rs.randint(0, 65536, size=(H, W)).astype(np.uint16)
    planes = [smooth, noisy, smooth]
    cfgs = [_cfg(40, grid, 1), _cfg(0, grid, 2), _cfg(40, grid, 3)]
    aligned = [0, (smooth.nbytes + 15) // 16 * 16]
    aligned.append(aligned[1] + (noisy.nbytes + 15) // 16 * 16 + 6)   # the third plane: 2-byte aligned only
    got, _ = _run(planes, cfgs, offsets=aligned)
    for b in range(3):
        assert got[b] is not None and np.array_equal(got[b], _want(planes[b], cfgs[b])), (shape, grid, b)


def test_batch_of_different_sizes_and_options():
    planes = [X.plane(37, 53, 1), X.plane(40, 64, 2), X.plane(2 * TILE_H + 1, 260, 3)]
    own = (100.0, 101.0, 102.0, 103.0)
    cfgs = [dict(_cfg(25), table=None),                               # grid = -1
            _cfg(-1, (2, 2), 4),                                      # dpc = -1
            dict(black=own, scale=X.scales(own, 16000.0, BLACK_OUT, WHITE_OUT), black_out=BLACK_OUT, dpc=10,
                 table=X.table(5, 7, 5))]                             # its own levels
    offsets, pos = [], 0
    for b, p in enumerate(planes):
        pos = (pos + 15) // 16 * 16 + (10 if b == 1 else 0)
        offsets.append(pos)
        pos += p.nbytes
    got, rec = _run(planes, cfgs, offsets=offsets)
    assert rec[0]["grid"] == -1 and rec[1]["dpc"] == -1 and rec[2]["grid"] > 0
    for b in range(3):
        assert np.array_equal(got[b], _want(planes[b], cfgs[b])), b
    # source and destination at different alignments
    got, _ = _run(planes, cfgs, offsets=offsets, dst_offsets=[o + 2 * (b + 1) for b, o in enumerate(offsets)])
    for b in range(3):
        assert np.array_equal(got[b], _want(planes[b], cfgs[b])), b


# ------------------------------------------------------------------------------------------------------------ hand-placed
def test_hand_placed_defects_ties_and_clips():
    defect_cases, tie_case, clip_case = X.defect_cases, X.tie_case, X.clip_case
    planes, cfgs = [], []
    for p, dpc, _ in defect_cases():
        planes.append(p)
        cfgs.append(dict(dpc=dpc))
    for p, c, _ in (tie_case(), clip_case()):
        planes.append(p)
        cfgs.append(c)
    got, _ = _run(planes, cfgs)
    for b, (p, c) in enumerate(zip(planes, cfgs)):
        assert np.array_equal(got[b], _want(p, c)), b
    for b, (_, _, want) in enumerate(defect_cases() + [tie_case(), clip_case()]):
        assert np.array_equal(got[b], want), b                        # and the values written down by hand


def test_identity_is_a_byte_copy():
    planes = [np.random.RandomState(s).randint(0, 65536, size=hw).astype(np.uint16)
              for s, hw in enumerate([(37, 53), (2, 2), (20, 2 * TILE_W + 1)])]
    cfgs = [dict(black=(64.0,) * 4, black_out=64.0), dict(), dict(black=BLACK[:1] * 4, black_out=BLACK[0])]
    got, _ = _run(planes, cfgs, offsets=[0, 3936, 3936 + 16 + 6])
    for b, p in enumerate(planes):
        assert np.array_equal(got[b], p), b


# ------------------------------------------------------------------------------------------------------------ bounds
def test_invalid_descriptors_are_skipped():
    planes = [X.plane(37, 53, 1), X.plane(40, 64, 2), X.plane(33, 47, 3), X.plane(9, 40, 4), X.plane(20, 30, 5)]
    cfgs = [_cfg(40, (5, 7), b) for b in range(5)]
    want = [_want(p, c) for p, c in zip(planes, cfgs)]

    def offset_out_of_range(rec):
        rec[1]["src_offset"] = 1 << 40

    def side_of_one(rec):
        rec[3]["src_w"] = 1

    def odd_offset(rec):
        rec[2]["dst_offset"] += 1

    def scale_not_finite(rec):
        rec[0]["scale"][2] = np.inf

    def grid_side_of_one(rec):
        rec[4]["grid_h"] = 1

    for mutate, bad in ((offset_out_of_range, 1), (side_of_one, 3), (odd_offset, 2), (scale_not_finite, 0),
                        (grid_side_of_one, 4)):
        got, _ = _run(planes, cfgs, mutate=mutate)
        for b in range(5):
            if b == bad:
                assert got[b] is None, (mutate.__name__, b)            # its sentinel bytes untouched
            else:
                assert np.array_equal(got[b], want[b]), (mutate.__name__, b)
    got, _ = _run(planes, cfgs, gain_cut=1)                           # the last table one word outside `gains`
    assert got[4] is None and all(np.array_equal(got[b], want[b]) for b in range(4))
    nogrid = [dict(c, table=None) for c in cfgs]
    got, rec = _run(planes, nogrid)                                   # no table anywhere: gains None
    assert all(np.array_equal(got[b], _want(planes[b], nogrid[b])) for b in range(5))


def test_argument_checks_on_the_device_side_of_the_binding():
    p = X.plane(8, 8, 1)
    rec = np.zeros(1, _lib.RAWFIX_DESC)
    fill_rawfix(rec[0], p.shape, 0, 0, (0,) * 4, (1,) * 4, 0.0, -1, None)
    src, desc = _dev(p.reshape(-1).view(np.uint8)), _dev(rec.view(np.uint8))
    with pytest.raises(_lib.AdaispError):
        _lib.raw_correct(src.cpu(), desc)
    with pytest.raises(_lib.AdaispError):
        _lib.raw_correct(src, desc[:-1])
    with pytest.raises(_lib.AdaispError):
        _lib.raw_correct(src, desc, out=src)                          # in place
    with pytest.raises(_lib.AdaispError):
        _lib.raw_correct(src, desc, gains=torch.zeros(16, dtype=torch.float64, device=DEV))
    out = torch.zeros(p.nbytes, dtype=torch.uint8, device=DEV)
    v = out._version
    _lib.raw_correct(src, desc, out=out)
    assert out._version > v and np.array_equal(out.cpu().numpy().view(np.uint16).reshape(p.shape), p)
