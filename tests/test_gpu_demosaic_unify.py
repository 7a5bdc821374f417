"""The whole-frame and the rectangle instantiation of the demosaic kernel are the same function of the plane, on a frame
that is not a whole number of tiles: S = 162 is two tile columns (128 + 34) and six tile rows (5 x 32 + 2), so the last
tile row is one cell row and the last tile column is partial. tests/test_gpu_bayer.py and tests/test_gpu_mhc.py compare
the two only on single-tile or exactly tiled frames."""
import numpy as np
import pytest
import torch

import _bayerref as R
import _mhcref as M
from adaptiveisp_amd import _lib

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
S, B, BLACK, WHITE = 162, 2, 64, 4095
PATTERNS = ("RGGB", "GRBG", "GBRG", "BGGR")
RECT_REF = {"bilinear": R.demosaic_rect, "mhc": M.mhc_rect}


def _desc(h, w, top, left):
    d = np.zeros(B, _lib.UNPROCESS_DESC)
    d["h"], d["w"], d["top"], d["left"] = h, w, top, left
    return torch.from_numpy(d.view(np.uint8).copy()).to(DEV)


@pytest.fixture(scope="module")
def plane():
    return np.random.RandomState(162).randint(0, 4200, size=(B, S, S)).astype(np.uint16)    # below black, above white


@pytest.mark.parametrize("method", ["bilinear", "mhc"])
def test_whole_frame_is_the_rectangle_that_fills_it(plane, method):
    raw = torch.from_numpy(plane.view(np.int16)).to(DEV)
    full = _desc(S, S, 0, 0)
    n = B * 3 * S * S
    for pattern in PATTERNS:
        kw = dict(pattern=pattern, black_level=BLACK, white_level=WHITE, method=method)
        whole = _lib.demosaic(raw, **kw)
        assert torch.equal(whole, _lib.demosaic_rects(raw, full, **kw)), pattern
        # one float off 8-byte alignment: the per-sample store path
        buf = torch.full((n + 3,), float("nan"), device=DEV)
        assert buf.data_ptr() % 8 == 0
        buf[0], buf[n + 1:] = 1234.5, -777.0
        out = buf[1:n + 1].view(B, 3, S, S)
        _lib.demosaic_rects(raw, full, out=out, **kw)
        assert torch.equal(out, whole), pattern
        assert buf[0].item() == 1234.5 and (buf[n + 1:] == -777.0).all(), pattern


@pytest.mark.parametrize("method", ["bilinear", "mhc"])
def test_rectangle_across_tile_edges_on_all_four_sides(oracle_mod, plane, method):
    h, w, top, left = 97, 131, 33, 29
    raw = torch.from_numpy(plane.view(np.int16)).to(DEV)
    pad = np.ones((S, S), bool)
    pad[top:top + h, left:left + w] = False
    for pattern in PATTERNS:
        got = _lib.demosaic_rects(raw, _desc(h, w, top, left), pattern=pattern, black_level=BLACK, white_level=WHITE,
                                  method=method).cpu().numpy()
        for b in range(B):
            want = RECT_REF[method](plane[b], h, w, top, left, pattern, BLACK, WHITE)
            assert np.array_equal(got[b], want), (pattern, b, int((got[b] != want).sum()))
            assert (got[b][:, pad] == 0).all(), (pattern, b)
