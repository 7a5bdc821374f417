"""Host side of the gradient-corrected (Malvar-He-Cutler) demosaic: the float64 restatement (tests/_mhcref.py) against
what defines the filters (impulse responses written out, constant colours, ramps, small and odd planes), its gain over
the bilinear oracle, the C entries' argument checks and binding, and the option on the source and the two command lines.
The kernels are checked against the restatement on the device by tests/test_gpu_mhc.py."""
import ctypes
import os

import numpy as np
import pytest
import torch

import _mhcref as M
import _unprocessref as U
from adaptiveisp_amd import _lib
from adaptiveisp_amd.data import ImageFolderSource

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PATTERNS = ("RGGB", "GRBG", "GBRG", "BGGR")


# ---------------------------------------------------------------------------------------------- the filters
def _impulse(y, x, pattern="RGGB"):
    """The 5 x 5 neighbourhood of the response to one sample of value 8 at (y, x) of a 12 x 12 plane (black 0, white 1),
    and whether everything outside that neighbourhood is 0."""
    plane = np.zeros((12, 12), np.uint16)
    plane[y, x] = 8
    out = M.mhc(plane, pattern, 0, 1)
    near = out[:, y - 2:y + 3, x - 2:x + 3].copy()
    out[:, y - 2:y + 3, x - 2:x + 3] = 0
    return near, not out.any()


def _grid(centre, ring1=(0, 0, 0), ring2=(0, 0)):
    """5 x 5: `centre`; ring1 = (W / E, N / S, the four diagonals) at distance 1; ring2 = (W2 / E2, N2 / S2)."""
    g = np.zeros((5, 5), np.float32)
    g[2, 2] = centre
    g[2, 1] = g[2, 3] = ring1[0]
    g[1, 2] = g[3, 2] = ring1[1]
    g[1, 1] = g[1, 3] = g[3, 1] = g[3, 3] = ring1[2]
    g[2, 0] = g[2, 4] = ring2[0]
    g[0, 2] = g[4, 2] = ring2[1]
    return g


def test_impulse_response_at_a_red_site():
    near, clean = _impulse(4, 6)
    assert clean
    red = np.zeros((5, 5), np.float32)
    red[1:4, 1:4] = [[2, 4, 2], [4, 8, 4], [2, 4, 2]]
    assert np.array_equal(near[0], red)
    assert np.array_equal(near[1], np.array([[0, 0, -1, 0, 0], [0, 0, 0, 0, 0], [-1, 0, 4, 0, -1], [0, 0, 0, 0, 0],
                                             [0, 0, -1, 0, 0]], np.float32))
    assert np.array_equal(near[2], np.array([[0, 0, -1.5, 0, 0], [0, 0, 0, 0, 0], [-1.5, 0, 6, 0, -1.5], [0, 0, 0, 0, 0],
                                             [0, 0, -1.5, 0, 0]], np.float32))
    # a blue site: the same with red and blue exchanged
    nb, clean = _impulse(5, 7)
    assert clean and np.array_equal(nb[2], near[0]) and np.array_equal(nb[1], near[1]) and np.array_equal(nb[0], near[2])


def test_impulse_response_at_the_green_sites():
    # green in a red row (red lies W / E, blue N / S)
    near, clean = _impulse(4, 7)
    assert clean
    assert np.array_equal(near[1], np.array([[0, 0, 0, 0, 0], [0, 0, 2, 0, 0], [0, 2, 8, 2, 0], [0, 0, 2, 0, 0],
                                             [0, 0, 0, 0, 0]], np.float32))
    assert np.array_equal(near[0], np.array([[0, 0, 0.5, 0, 0], [0, -1, 0, -1, 0], [-1, 0, 5, 0, -1], [0, -1, 0, -1, 0],
                                             [0, 0, 0.5, 0, 0]], np.float32))
    assert np.array_equal(near[2], np.array([[0, 0, -1, 0, 0], [0, -1, 0, -1, 0], [0.5, 0, 5, 0, 0.5], [0, -1, 0, -1, 0],
                                             [0, 0, -1, 0, 0]], np.float32))
    assert np.array_equal(near[0], _grid(5, (0, 0, -1), (-1, 0.5))) and np.array_equal(near[2], _grid(5, (0, 0, -1), (0.5, -1)))
    # green in a blue row: red and blue exchanged
    nb, clean = _impulse(5, 6)
    assert clean and np.array_equal(nb[1], near[1]) and np.array_equal(nb[0], near[2]) and np.array_equal(nb[2], near[0])


def _mosaic(rgb_hwc, pattern):
    """[h, w] plane of an integer [h, w, 3] image: every pixel keeps the channel its site samples."""
    h, w = rgb_hwc.shape[:2]
    pat = M.CFA[pattern]
    py, px = (np.arange(h)[:, None] - (pat >> 1)) & 1, (np.arange(w)[None, :] - (pat & 1)) & 1
    ch = np.where(py == px, 2 * py, 1)
    return np.take_along_axis(rgb_hwc, ch[..., None], axis=-1)[..., 0]


def _norm(v, black, white):
    return (np.asarray(v, np.float32) - np.float32(black)) * (np.float32(1) / (np.float32(white) - np.float32(black)))


@pytest.mark.parametrize("pattern", PATTERNS)
def test_constant_colour_comes_back_constant(pattern):
    rgb = np.array([900, 2500, 301])
    plane = _mosaic(np.broadcast_to(rgb, (9, 11, 3)), pattern).astype(np.uint16)
    out = M.mhc(plane, pattern, 64, 4095)
    for c in range(3):
        assert (out[c] == _norm(rgb[c], 64, 4095)).all(), (pattern, c)


@pytest.mark.parametrize("pattern", PATTERNS)
def test_ramps_come_back_exact_away_from_the_border(pattern):
    y, x = np.mgrid[0:12, 0:14]
    img = np.stack([100 + 7 * x + 3 * y, 2000 - 5 * x + 11 * y, 640 + 2 * x - 9 * y + 200], axis=-1)
    assert img.min() >= 64 and img.max() <= 4095
    out = M.mhc(_mosaic(img, pattern).astype(np.uint16), pattern, 64, 4095)
    want = _norm(img.transpose(2, 0, 1), 64, 4095)
    assert np.array_equal(out[:, 2:-2, 2:-2], want[:, 2:-2, 2:-2])
    assert not np.array_equal(out, want)                                     # the mirror bends a ramp at the border


@pytest.mark.parametrize("h,w", [(2, 2), (2, 5), (3, 3), (5, 7)])
def test_small_and_odd_planes_keep_their_samples(h, w):
    rs = np.random.RandomState(10 * h + w)
    plane = rs.randint(0, 4200, size=(h, w)).astype(np.uint16)
    for pattern in PATTERNS:
        out = M.mhc(plane, pattern, 64, 4095)
        assert out.shape == (3, h, w) and out.dtype == np.float32 and np.isfinite(out).all()
        site = _mosaic(np.broadcast_to(np.arange(3), (h, w, 3)), pattern)
        got = np.take_along_axis(out, site[None], axis=0)[0]
        assert np.array_equal(got, _norm(plane, 64, 4095)), pattern
    S = 9
    frame = np.zeros((S, S), np.uint16)
    frame[1:1 + h, 2:2 + w] = plane
    r = M.mhc_rect(frame, h, w, 1, 2, "GRBG", 64, 4095)
    assert np.array_equal(r[:, 1:1 + h, 2:2 + w], M.mhc(plane, "GRBG", 64, 4095))
    r[:, 1:1 + h, 2:2 + w] = 0
    assert not r.any()
    assert not M.mhc_rect(frame, 1, w, 1, 2).any() and not M.mhc_rect(frame, h, 1, 1, 2).any()
    assert not M.mhc_rect(frame, h, w, S - h + 1, 0).any() and not M.mhc_rect(frame, h, w, 0, -1).any()


def test_double_fold_on_a_two_pixel_side():
    # period 2n - 2 = 2: index -2 -> 0, -1 -> 1, 2 -> 0, 3 -> 1
    plane = np.array([[100, 300], [700, 1500]], np.uint16)
    tiled = np.tile(plane, (3, 3))
    for pattern in PATTERNS:
        assert np.array_equal(M.mhc(plane, pattern, 0, 4095), M.mhc(tiled, pattern, 0, 4095)[:, 2:4, 2:4])


# ---------------------------------------------------------------------------------------------- quality
def _luminances():
    y, x = np.mgrid[0:64, 0:64].astype(np.float64)
    chirp = 0.5 + 0.4 * np.cos(np.pi * x * x / 256 + 0 * y)                  # local period 512 / x: down to 8 px at x = 63
    edge = 0.1 + 0.8 * np.clip((x - 32) + 0.2 * (y - 32) + 0.5, 0, 1)         # one pixel wide, ~ 11 degrees off the vertical
    sine = 0.5 + 0.35 * np.sin(2 * np.pi * (x + y) / 7)                       # period 7 along x + y
    return dict(chirp=chirp, edge=edge, sine=sine)


@pytest.mark.parametrize("name", ["chirp", "edge", "sine"])
def test_mhc_beats_the_bilinear_oracle(oracle_mod, name):
    """Interior RMSE against the un-mosaiced image, channels = luminance x (0.9, 1, 0.7), 12 bits over black 64: the
    bilinear oracle's is at least 1.5 x the restatement's. The three images are this test's own definitions
    (_luminances), not those of an earlier experiment: on them the gain is chirp 2.42-2.50 x, edge 1.73-1.74 x, sine
    1.94 x."""
    black, white = 64, 4095
    lum = _luminances()[name]
    truth = lum[..., None] * np.array([0.9, 1.0, 0.7])
    img = np.rint(truth * (white - black)).astype(np.int64) + black
    want = ((img - black) / (white - black)).transpose(2, 0, 1)
    for pattern in PATTERNS:
        plane = _mosaic(img, pattern).astype(np.uint16)
        bil = oracle_mod.demosaic(plane[None], M.CFA[pattern], black, white)[0].astype(np.float64)
        mhc = M.mhc(plane, pattern, black, white).astype(np.float64)
        rm = lambda a: np.sqrt(((a - want)[:, 4:-4, 4:-4] ** 2).mean())       # noqa: E731
        print(f"{name} {pattern}: rmse bilinear {rm(bil):.5f} mhc {rm(mhc):.5f} ratio {rm(bil) / rm(mhc):.2f}")
        assert rm(mhc) <= rm(bil) / 1.5, (name, pattern, rm(bil), rm(mhc))


# ---------------------------------------------------------------------------------------------- C entries and binding
def test_header_and_exports_declare_the_entries():
    hdr = open(os.path.join(ROOT, "include", "adaisp.h")).read()
    assert "int adaisp_demosaic_ex(" in hdr and "int adaisp_demosaic_rects_ex(" in hdr
    assert "#define ADAISP_DEMOSAIC_BILINEAR 0" in hdr and "#define ADAISP_DEMOSAIC_MHC      1" in hdr
    assert "#define ADAISP_ABI_VERSION 9" in hdr
    assert "adaisp_demosaic_ex" in _lib.EXPORTS and "adaisp_demosaic_rects_ex" in _lib.EXPORTS
    assert _lib.DEMOSAIC == {"bilinear": 0, "mhc": 1} and _lib.ABI_VERSION == 9
    L = _lib.load()
    assert L.adaisp_abi_version() == 9
    assert hasattr(L, "adaisp_demosaic_ex") and hasattr(L, "adaisp_demosaic_rects_ex")


def test_cabi_rejects_bad_arguments():
    L = _lib.load()
    p = ctypes.c_void_p(16)
    E, SH = -1, -4

    def whole(raw=p, out=p, B=1, S=8, pattern=0, method=1, black=64.0, white=1023.0):
        return L.adaisp_demosaic_ex(raw, out, B, S, S, pattern, method, black, white, None)

    def rects(raw=p, desc=p, out=p, B=1, S=8, pattern=0, method=1, black=64.0, white=1023.0):
        return L.adaisp_demosaic_rects_ex(raw, desc, out, B, S, pattern, method, black, white, None)

    assert rects(desc=None) == E and rects(desc=None, method=0) == E
    for f in (whole, rects):
        for m in (0, 1):
            assert f(raw=None, method=m) == E and f(out=None, method=m) == E
            assert f(B=0, method=m) == E and f(B=-1, method=m) == E and f(S=0, method=m) == E and f(S=-3, method=m) == E
            assert f(pattern=4, method=m) == E and f(pattern=-1, method=m) == E
            assert f(black=1023.0, method=m) == E and f(black=2000.0, method=m) == E
            assert f(white=float("nan"), method=m) == E and f(black=float("nan"), method=m) == E
            assert f(B=65536, method=m) == SH
        assert f(method=-1) == E and f(method=2) == E
    assert rects(S=32769) == SH and rects(S=32769, method=0) == SH
    assert whole(S=7) == SH                                                  # whole frame: H and W even, as adaisp_demosaic


def test_wrappers_reject_host_tensors_and_unknown_methods():
    desc = torch.zeros(_lib.UNPROCESS_DESC.itemsize, dtype=torch.uint8)
    raw = torch.zeros((1, 4, 4), dtype=torch.int16)
    for method in ("bilinear", "mhc"):
        with pytest.raises(_lib.AdaispError, match="HIP device"):
            _lib.demosaic(raw, method=method)
        with pytest.raises(_lib.AdaispError, match="HIP device"):
            _lib.demosaic_rects(raw, desc, method=method)
    for bad in ("nope", "MHC", 1, None):
        with pytest.raises(_lib.AdaispError, match="method"):
            _lib.demosaic(raw, method=bad)
        with pytest.raises(_lib.AdaispError, match="method"):
            _lib.demosaic_rects(raw, desc, method=bad)


class _SaysDevice(torch.Tensor):
    """A host tensor whose `device` says cuda:0: it gets the arguments before the one under test past their own device check
    on a machine without a device (nothing is launched: the argument under test raises first)."""
    @property
    def device(self):
        return torch.device("cuda:0")


def test_every_front_end_wrapper_names_the_host_tensor_it_was_given():
    """Each tensor argument of the seven front-end wrappers in turn is a host tensor, the others pass for device tensors:
    AdaispError naming the wrapper, the argument and what it must be, before any device work."""
    def u8(n):
        return torch.zeros(n, dtype=torch.uint8)
    plane = torch.zeros((1, 4, 4), dtype=torch.int16)
    rec = np.zeros(1, _lib.RESIZE_DESC)
    rec["src_h"], rec["src_w"], rec["dst_h"], rec["dst_w"] = 2, 2, 2, 2
    f32 = torch.float32
    calls = {
        "unprocess": (lambda src, desc, out: _lib.unprocess(src, desc, 4, out=out),
                      dict(src=u8(48), desc=u8(_lib.UNPROCESS_DESC.itemsize), out=torch.zeros((1, 3, 4, 4), dtype=f32))),
        "unprocess_bayer": (lambda src, desc, out: _lib.unprocess_bayer(src, desc, 4, out=out),
                            dict(src=u8(48), desc=u8(_lib.UNPROCESS_DESC.itemsize), out=plane.clone())),
        "demosaic": (lambda raw, out: _lib.demosaic(raw, out=out),
                     dict(raw=plane.clone(), out=torch.zeros((1, 3, 4, 4), dtype=f32))),
        "demosaic_rects": (lambda raw, desc, out: _lib.demosaic_rects(raw, desc, out=out),
                           dict(raw=plane.clone(), desc=u8(_lib.UNPROCESS_DESC.itemsize),
                                out=torch.zeros((1, 3, 4, 4), dtype=f32))),
        "resize_u8": (lambda src, dst, desc, tabs: _lib.resize_u8(src, dst, desc, tabs, rec),
                      dict(src=u8(12), dst=u8(12), desc=u8(rec.nbytes), tabs=torch.zeros(8, dtype=torch.int32))),
        "raw_load": (lambda src, desc, tabs, out: _lib.raw_load(src, desc, tabs, 4, out=out),
                     dict(src=u8(32), desc=u8(_lib.RAW_DESC.itemsize), tabs=torch.zeros(8, dtype=torch.int32),
                          out=torch.zeros((1, 3, 4, 4), dtype=f32))),
        "raw_correct": (lambda src, desc, gains, out: _lib.raw_correct(src, desc, gains, out=out),
                        dict(src=u8(32), desc=u8(_lib.RAWFIX_DESC.itemsize), gains=torch.zeros(4, dtype=f32), out=u8(32))),
    }
    for wrapper, (call, args) in calls.items():
        for bad in args:
            given = {k: v if k == bad else v.as_subclass(_SaysDevice) for k, v in args.items()}
            with pytest.raises(_lib.AdaispError) as e:
                call(**given)
            text = str(e.value)
            assert wrapper + ":" in text and f" {bad} " in text and "HIP device" in text, (wrapper, bad, text)


# ---------------------------------------------------------------------------------------------- options
def test_source_validates_the_demosaic(tmp_path):
    U.write_dataset(str(tmp_path), [(12, 10), (9, 14)], seed=1)
    for bad in ("nope", "MHC", None, 1):
        with pytest.raises(ValueError, match="demosaic"):
            ImageFolderSource(str(tmp_path), 64, "cpu", workers=0, demosaic=bad)
    with pytest.raises(RuntimeError, match="sensor='bayer'"):                # the sensor itself still needs the device
        ImageFolderSource(str(tmp_path), 64, "cpu", workers=0, sensor="bayer", demosaic="mhc")
    for kw, dm in ((dict(), "bilinear"), (dict(demosaic="mhc"), "mhc")):
        src = ImageFolderSource(str(tmp_path), 64, "cpu", workers=0, **kw)
        try:
            assert src.demosaic == dm and src.describe() == "lod: 2 files"    # no meaning without sensor="bayer"
        finally:
            src.close()


def test_clis_parse_the_demosaic_option():
    from adaptiveisp_amd.train import build_parser
    from adaptiveisp_amd.val.__main__ import build_parser as val_parser
    base = ["--isp-ckpt", "x.pth", "--data", "d"]
    for ap, extra in ((build_parser(), []), (val_parser(), base)):
        assert ap.parse_args(extra).demosaic == "bilinear"
        a = ap.parse_args(extra + ["--sensor", "bayer", "--demosaic", "mhc"])
        assert (a.sensor, a.demosaic) == ("bayer", "mhc")
        for bad in ("nope", "MHC", "malvar"):
            with pytest.raises(SystemExit):
                ap.parse_args(extra + ["--demosaic", bad])
        assert "--demosaic" in ap.format_help()
