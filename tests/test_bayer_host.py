"""Host side of the simulated Bayer sensor: the float64 restatement (tests/_bayerref.py) against the reference's fixture
(tests/golden/bayer.npz), the quantiser, the colour-filter maps, the C entries' argument checks and binding, and the
options of the source and the two command lines. The kernels are checked on the device by tests/test_gpu_bayer.py."""
import ctypes
import os

import numpy as np
import pytest
import torch

import _bayerref as R
import _unprocessref as U
from adaptiveisp_amd import _lib
from adaptiveisp_amd.data import ImageFolderSource

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _cases(z):
    k = 0
    while f"case{k}.plane" in z.files:
        yield f"case{k}."
        k += 1
    yield "sat."


def test_restatement_reproduces_the_reference_planes(golden):
    z = golden("bayer")
    names = list(_cases(z))
    assert len(names) >= 7
    for c in names:
        img, plane = z[c + "img"], z[c + "plane"]
        assert img.dtype == np.uint8 and img.shape[0] % 2 == 0 and img.shape[1] % 2 == 0
        assert img.shape[0] <= 32 and img.shape[1] <= 48 and plane.shape == img.shape[:2] and plane.dtype == np.float64
        got = R.sensor_plane(img, z[c + "rgb2cam"], *z[c + "gains"], pattern="RGGB")
        assert np.abs(got - plane).max() <= 1e-12, c
    # the saturation case reaches safe_invert_gains' mask
    assert (U.saturation_mask(z["sat.img"], z["sat.rgb2cam"]) > 0.05).sum() >= 10


def test_quantiser_rounds_half_to_even_and_clamps():
    for dt in (np.float64, np.float32):
        q = lambda v, b, w: R.quantise(np.array(v, dt), b, w)                # noqa: E731
        assert q([0.0, 1.0], 64, 1023).tolist() == [64, 1023]
        assert q([0.0, 1.0], 0, 65535).tolist() == [0, 65535]
        # half an LSB is a tie: to the even count (0.5 / 2 -> 0, 1.5 / 2 -> 2), then the black level is added
        assert q([0.25, 0.75], 10, 12).tolist() == [10, 12]
        assert q([0.5 / 1024, 1.5 / 1024, 2.5 / 1024], 64, 1088).tolist() == [64, 66, 66]
        # a white level past 16 bits and a negative sample saturate
        assert q([1.0, -1.0], 60000, 70000).tolist() == [65535, 50000]
        assert q([-1.0], 100, 4095).tolist() == [0]
    assert R.quantise(np.float32(0.3), 256, 4095).dtype == np.uint16


def test_cfa_maps_follow_the_reference_packing(golden):
    z = golden("bayer")
    for name, pat in R.CFA.items():
        ref = z["cfa." + name]
        assert np.array_equal(R.cfa_channels(*ref.shape, name), ref), name
        assert np.array_equal(R.cfa_channels(*ref.shape, pat), ref), name
        assert ref[pat >> 1, pat & 1] == 0 and ref[1 - (pat >> 1), 1 - (pat & 1)] == 2      # red, and blue across
        assert _lib.CFA[name] == pat
    # odd sizes keep the phase of the origin
    assert np.array_equal(R.cfa_channels(3, 5, "GBRG"), np.tile(z["cfa.GBRG"], (2, 2))[:3, :5])
    img = np.arange(4 * 6 * 3, dtype=np.float64).reshape(4, 6, 3)
    assert R.mosaic_plane(img, "RGGB")[1, 1] == img[1, 1, 2] and R.mosaic_plane(img, "BGGR")[0, 0] == img[0, 0, 2]


def test_rect_demosaic_restatement_pads_with_zeros_and_mirrors_inside(oracle_mod):
    rs = np.random.RandomState(0)
    plane = rs.randint(64, 4096, size=(16, 16)).astype(np.uint16)
    whole = R.demosaic_rect(plane, 16, 16, 0, 0, 1, 64, 4095)
    assert np.array_equal(whole, oracle_mod.demosaic(plane[None], 1, 64, 4095)[0])
    out = R.demosaic_rect(plane, 5, 7, 3, 5, 0, 64, 4095)
    pad = np.ones((16, 16), bool)
    pad[3:8, 5:12] = False
    assert (out[:, pad] == 0).all() and (out[:, ~pad] != 0).any()
    # at a red site the red output is the sample, whatever lies outside the rectangle
    assert out[0, 3, 5] == (np.float32(plane[3, 5]) - np.float32(64)) * (np.float32(1) / np.float32(4095 - 64))
    # the last (odd) row mirrors onto row h - 2: green at the red site (h - 1, 0) = ((N + N) + (E + E)) / 4
    s = (plane[3:8, 5:12].astype(np.float32) - np.float32(64)) * (np.float32(1) / np.float32(4095 - 64))
    assert out[1, 7, 5] == ((s[3, 0] + s[3, 0]) + (s[4, 1] + s[4, 1])) * np.float32(0.25)
    assert not R.demosaic_rect(plane, 1, 7, 0, 0).any() and not R.demosaic_rect(plane, 6, 6, 11, 0).any()


# ---------------------------------------------------------------------------------------------- C entries and binding
def test_header_and_exports_declare_the_entries():
    hdr = open(os.path.join(ROOT, "include", "adaisp.h")).read()
    assert "int adaisp_unprocess_bayer(" in hdr and "int adaisp_demosaic_rects(" in hdr
    assert "#define ADAISP_ABI_VERSION 9" in hdr
    assert "adaisp_unprocess_bayer" in _lib.EXPORTS and "adaisp_demosaic_rects" in _lib.EXPORTS
    assert _lib.ABI_VERSION == 9
    L = _lib.load()
    assert L.adaisp_abi_version() == 9
    for name in _lib.EXPORTS:
        assert hasattr(L, name), name


def test_cabi_rejects_bad_arguments():
    L = _lib.load()
    p = ctypes.c_void_p(16)
    E, SH = -1, -4
    NF = _lib.UNP_UNPROCESS | _lib.UNP_NOISE

    def sensor(src=p, desc=p, out=p, B=1, S=8, flags=0, pattern=0, black=64.0, white=1023.0):
        return L.adaisp_unprocess_bayer(src, desc, out, B, S, 0, flags, pattern, black, white, None)

    def rects(raw=p, desc=p, out=p, B=1, S=8, pattern=0, black=64.0, white=1023.0):
        return L.adaisp_demosaic_rects(raw, desc, out, B, S, pattern, black, white, None)

    assert sensor(src=None) == E and sensor(desc=None) == E and sensor(out=None) == E
    assert rects(raw=None) == E and rects(desc=None) == E and rects(out=None) == E
    for f in (sensor, rects):
        assert f(B=0) == E and f(B=-1) == E and f(S=0) == E and f(S=-3) == E
        assert f(pattern=4) == E and f(pattern=-1) == E
        assert f(black=1023.0) == E and f(black=2000.0) == E and f(white=float("nan")) == E
        assert f(B=65536) == SH and f(S=32769) == SH
    assert sensor(flags=_lib.UNP_NOISE) == E and sensor(flags=4) == E and sensor(flags=NF | 8) == E


def test_wrappers_reject_host_tensors():
    desc = torch.zeros(_lib.UNPROCESS_DESC.itemsize, dtype=torch.uint8)
    with pytest.raises(_lib.AdaispError):
        _lib.unprocess_bayer(torch.zeros(64, dtype=torch.uint8), desc, 4)
    with pytest.raises(_lib.AdaispError):
        _lib.demosaic_rects(torch.zeros((1, 4, 4), dtype=torch.int16), desc)


# ---------------------------------------------------------------------------------------------- options
@pytest.fixture(scope="module")
def toy(tmp_path_factory):
    root = tmp_path_factory.mktemp("bayerds")
    U.write_dataset(str(root), [(12, 10), (9, 14)], seed=1)
    return str(root)


def test_bayer_source_needs_the_device_and_valid_options(toy):
    with pytest.raises(RuntimeError, match="sensor='bayer'"):
        ImageFolderSource(toy, 64, "cpu", sensor="bayer", workers=0)
    for kw in (dict(sensor="raw"), dict(sensor=None), dict(cfa="RGBG"), dict(cfa=0), dict(raw_bits=0), dict(raw_bits=17),
               dict(raw_bits=12.5), dict(raw_bits="12"), dict(black_level=4095), dict(black_level=-1),
               dict(sensor="bayer", cfa="XYZW"), dict(sensor="bayer", raw_bits=20)):
        with pytest.raises(ValueError):
            ImageFolderSource(toy, 64, "cpu", workers=0, **kw)
    src = ImageFolderSource(toy, 64, "cpu", workers=0)                       # the default stays the rgb path
    try:
        assert src.sensor == "rgb" and "bayer" not in src.describe() and src.describe() == "lod: 2 files"
        assert (src.cfa, src.raw_bits, src.white_level, src.black_level) == ("RGGB", 12, 4095, 64)
    finally:
        src.close()
    for bits, black in ((12, 64), (10, 16), (16, 1024), (6, 1), (5, 0), (1, 0)):
        src = ImageFolderSource(toy, 64, "cpu", workers=0, raw_bits=bits, cfa="grbg")
        assert (src.white_level, src.black_level, src.cfa) == (2 ** bits - 1, black, "GRBG")
        src.close()
    src = ImageFolderSource(toy, 64, "cpu", workers=0, raw_bits=10, black_level=64)
    assert src.black_level == 64
    src.close()


def test_clis_parse_the_sensor_options():
    from adaptiveisp_amd.train import build_parser
    from adaptiveisp_amd.val.__main__ import build_parser as val_parser
    base = ["--isp-ckpt", "x.pth", "--data", "d"]
    for ap, extra in ((build_parser(), []), (val_parser(), base)):
        a = ap.parse_args(extra)
        assert (a.sensor, a.cfa, a.raw_bits, a.black_level) == ("rgb", "RGGB", 12, None)
        a = ap.parse_args(extra + ["--sensor", "bayer", "--cfa", "BGGR", "--raw-bits", "10", "--black-level", "64"])
        assert (a.sensor, a.cfa, a.raw_bits, a.black_level) == ("bayer", "BGGR", 10, 64)
        for bad in (["--sensor", "raw"], ["--cfa", "RGBG"], ["--raw-bits", "x"]):
            with pytest.raises(SystemExit):
                ap.parse_args(extra + bad)
        assert "--sensor" in ap.format_help()
