"""The host half of the raw-capture loader (adaisp_raw_load), without a GPU: the fp32 tap tables of
adaptiveisp_amd/resize.py, the numpy definition of the kernel's output (tests/_rawref.py) against the float64 product of
the same weights, the package (header, exports, descriptor layout), the C-ABI's argument checks, the two command lines
and the construction of ImageFolderSource(data_name="raw")."""
import ctypes
import os
import re

import numpy as np
import pytest

import _rawref as R
import _resizeref
from adaptiveisp_amd import _lib
from adaptiveisp_amd.resize import RawTapPlan, area_table, identity_table, linear_table_f32, raw_table
from adaptiveisp_amd.val.loader import IMG_FORMATS, _linear_taps, list_images

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PATTERNS = ("RGGB", "GRBG", "GBRG", "BGGR")
SHAPES = [((2, 2), (2, 2)), ((7, 9), (4, 5)), ((37, 53), (16, 23)), ((64, 96), (16, 24)), ((300, 520), (20, 35)),
          ((10, 14), (23, 32))]


# ------------------------------------------------------------------------------------------------------------ tap tables
@pytest.mark.parametrize("src,dst", [(10, 23), (14, 32), (3, 300), (20, 33), (2, 3), (511, 512), (1, 4)])
def test_linear_table_f32(src, dst):
    ptr, idx, wt = _resizeref._csr(linear_table_f32(src, dst), dst)
    cnt = np.diff(ptr)
    assert cnt.min() >= 1 and cnt.max() <= 2 and ptr[0] == 0
    assert idx.min() >= 0 and idx.max() < src and (wt >= 0).all()
    sums = np.array([wt[ptr[d]:ptr[d + 1]].astype(np.float64).sum() for d in range(dst)])
    assert np.abs(sums - 1.0).max() <= 2.0 ** -24                     # 1 ulp of fp32 below 1
    # the mapping of _linear_taps: same left index; the second tap (where there is one) is its right neighbour
    i0 = _linear_taps(src, dst)[0]
    assert np.array_equal(idx[ptr[:-1]], i0)
    two = cnt == 2
    assert np.array_equal(idx[ptr[:-1][two] + 1], i0[two] + 1)
    assert (wt[ptr[:-1][~two]] == 1.0).all()


def test_raw_table_picks_area_linear_or_identity():
    assert raw_table(53, 23) is area_table(53, 23)
    assert raw_table(14, 32) is linear_table_f32(14, 32)
    assert raw_table(9, 9) is identity_table(9)
    ptr, idx, wt = _resizeref._csr(raw_table(9, 9), 9)
    assert np.array_equal(ptr, np.arange(10)) and np.array_equal(idx, np.arange(9)) and (wt == 1.0).all()


def test_raw_tap_plan_shares_tables_and_fills_records():
    plan = RawTapPlan(base=5)
    plan.add((37, 53), (16, 23), (1, 3), 0)
    plan.add((37, 53), (16, 23), (0, 0), 4000, gains=(1.9, 1.0, 1.6))
    plan.add((53, 37), (23, 16), (2, 2), 8000)
    rec, tab = plan.descriptors(), plan.table()
    assert rec.dtype == _lib.RAW_DESC and len(rec) == 3
    assert rec[0]["tab_x"] == rec[1]["tab_x"] == 5 and rec[0]["tab_y"] == rec[1]["tab_y"] == rec[2]["tab_x"]
    assert rec[2]["tab_y"] == rec[0]["tab_x"]
    assert tab.size == raw_table(53, 23).size + raw_table(37, 16).size
    assert np.array_equal(tab[int(rec[0]["tab_y"]) - 5:][:raw_table(37, 16).size], raw_table(37, 16))
    assert rec[1]["gain"].tolist() == [np.float32(1.9), 1.0, np.float32(1.6)] and rec[0]["gain"].tolist() == [1.0] * 3
    assert (rec[1]["src_h"], rec[1]["src_w"], rec[1]["h"], rec[1]["w"], rec[0]["top"], rec[0]["left"]) == (37, 53, 16, 23, 1, 3)


# ------------------------------------------------------------------------------------------------------------ reference
def _bound(d, H, W, h, w):
    """K sequential fp32 multiply-adds of a convex combination: each of the kx + ky products and sums rounds once, by at
    most 2^-24 of a value no larger than max |D| (the weights are non-negative and sum to 1 within an ulp)."""
    return (R.max_taps(W, w) + R.max_taps(H, h) + 2) * 2.0 ** -24 * float(np.abs(d).max())


@pytest.mark.parametrize("pattern", PATTERNS)
@pytest.mark.parametrize("src_hw,dst_hw", SHAPES)
def test_definition_is_within_the_derived_bound_of_the_exact_product(src_hw, dst_hw, pattern):
    (H, W), (h, w) = src_hw, dst_hw
    p = R.plane(H, W, H * W)
    d = R.demosaic(p, pattern, "mhc", 64, 4095)
    got = R.raw_load_one(p, dst_hw, (0, 0), max(h, w), pattern, "mhc", 64, 4095)[:, :h, :w]
    err = float(np.abs(got.astype(np.float64) - R.exact(d, h, w)).max())
    assert err <= _bound(d, H, W, h, w), (err, _bound(d, H, W, h, w))


@pytest.mark.parametrize("method", ("bilinear", "mhc"))
def test_constant_plane_gives_a_constant_image(method):
    for (H, W), (h, w) in SHAPES:
        p = np.full((H, W), 1000, np.uint16)
        out = R.raw_load_one(p, (h, w), (1, 1), max(h, w) + 2, "GRBG", method, 64, 4095)
        level = np.float32(np.float32(1000 - 64) * (np.float32(1) / np.float32(4095 - 64)))
        inside = out[:, 1:1 + h, 1:1 + w]
        bound = (R.max_taps(W, w) + R.max_taps(H, h) + 2) * 2.0 ** -24 * float(level)
        assert np.abs(inside.astype(np.float64) - float(level)).max() <= bound
        outside = out.copy()
        outside[:, 1:1 + h, 1:1 + w] = 0
        assert not outside.any()


def test_degenerate_images_are_zero():
    p = R.plane(8, 8, 1)
    assert not R.raw_load_one(p, (4, 4), (6, 0), 8).any()                       # does not fit
    assert not R.raw_load_one(np.zeros((9, 1), np.uint16) + 9, (9, 1), (0, 0), 16).any()
    assert R.raw_load_one(p, (4, 4), (4, 4), 8).any()


# ------------------------------------------------------------------------------------------------------------ package
def _header():
    text = open(os.path.join(ROOT, "include", "adaisp.h")).read()
    return text, re.sub(r"/\*.*?\*/", "", text, flags=re.S)


def test_header_library_and_descriptor():
    text, code = _header()
    assert re.search(r"\bint\s+adaisp_raw_load\s*\(", code)
    assert "adaisp_raw_load" in _lib.EXPORTS
    L = _lib.load()
    assert hasattr(L, "adaisp_raw_load")
    assert re.search(r"#define\s+ADAISP_ABI_VERSION\s+9\b", text) and L.adaisp_abi_version() == 9 == _lib.ABI_VERSION

    class Desc(ctypes.Structure):                                     # the header's fields, in its order
        _fields_ = [("src_offset", ctypes.c_int64), ("src_h", ctypes.c_int32), ("src_w", ctypes.c_int32),
                    ("h", ctypes.c_int32), ("w", ctypes.c_int32), ("top", ctypes.c_int32), ("left", ctypes.c_int32),
                    ("tab_x", ctypes.c_int64), ("tab_y", ctypes.c_int64), ("gain", ctypes.c_float * 3),
                    ("reserved", ctypes.c_float)]
    body = re.search(r"typedef struct adaisp_raw_desc \{(.*?)\} adaisp_raw_desc;", code, flags=re.S).group(1)
    names = re.findall(r"(\w+)(?:\[\d+\])?\s*[,;]", body)
    assert names == [f[0] for f in Desc._fields_]
    # 8 + 6 * 4 + 2 * 8 + 4 * 4 bytes (adaisp_resize_desc, the other descriptor with taps, is 56)
    assert _lib.RAW_DESC.itemsize == ctypes.sizeof(Desc) == 64
    for name, _ in Desc._fields_:
        assert _lib.RAW_DESC.fields[name][1] == getattr(Desc, name).offset, name


def test_argument_checks_without_gpu():
    L = _lib.load()
    buf = (ctypes.c_float * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)

    def call(src=p, desc=p, tabs=p, out=p, B=1, S=8, pattern=0, method=1, black=64.0, white=4095.0, src_bytes=128, words=16):
        return L.adaisp_raw_load(src, src_bytes, desc, tabs, words, out, B, S, pattern, method, black, white, None)

    for null in ("src", "desc", "tabs", "out"):
        assert call(**{null: None}) == -1, null
    assert call(pattern=4) == -1 and call(pattern=-1) == -1
    assert call(method=2) == -1 and call(method=-1) == -1
    assert call(black=100.0, white=100.0) == -1 and call(black=200.0, white=100.0) == -1
    assert call(src=ctypes.c_void_p(p.value + 1)) == -1                 # uint16 samples at an odd address
    assert call(B=-1) == -1 and call(S=0) == -1
    assert call(B=65536) == -4 and call(S=32769) == -4
    assert call(B=0) == 0                                             # nothing to do, nothing launched


# ------------------------------------------------------------------------------------------------------------ CLIs
def test_cli_parsing(capsys):
    from adaptiveisp_amd import train
    from adaptiveisp_amd.val.__main__ import parse_args as val_args
    base = ["--isp-ckpt", "x.pth", "--data", "planes"]
    a = val_args(base + ["--data-name", "raw", "--cfa", "GBRG", "--raw-bits", "14", "--demosaic", "mhc", "--raw-gains", "1.9",
                         "1", "1.6"])
    assert a.data_name == "raw" and list(a.raw_gains) == [1.9, 1.0, 1.6] and (a.cfa, a.raw_bits, a.demosaic) == ("GBRG", 14, "mhc")
    assert list(val_args(base + ["--data-name", "raw"]).raw_gains) == [1.0, 1.0, 1.0]
    a = val_args(base + ["--data-name", "raw", "--add-noise", "--bri-range", "0.1", "0.5"])
    assert a.add_noise is False and a.bri_range is None and "ignored" in capsys.readouterr().out
    t = train.parse_args(["--data", "planes", "--data-name", "raw", "--raw-gains", "2", "1", "1.5", "--add-noise"])
    assert t.data_name == "raw" and list(t.raw_gains) == [2.0, 1.0, 1.5] and t.add_noise is False
    assert "ignored" in capsys.readouterr().out
    for parse, argv in ((val_args, base), (train.parse_args, ["--data", "planes"])):
        for bad in (["--data-name", "raw", "--sensor", "bayer"], ["--data-name", "raw", "--raw-gains", "1", "2"],
                    ["--data-name", "raw", "--raw-gains", "1", "2", "x"]):
            with pytest.raises(SystemExit) as e:
                parse(argv + bad)
            assert e.value.code == 2, bad
    capsys.readouterr()


# ------------------------------------------------------------------------------------------------------------ source
def _planes(tmp_path, arrays):
    d = tmp_path / "images"
    d.mkdir()
    for name, a in arrays.items():
        np.save(d / name, a)
    return str(d)


def test_list_images_formats(tmp_path):
    d = _planes(tmp_path, {"a.npy": np.zeros((4, 4), np.uint16)})
    open(os.path.join(d, "b.png"), "wb").close()
    assert [os.path.basename(f) for f in list_images(d)] == ["b.png"]            # the default is unchanged
    assert [os.path.basename(f) for f in list_images(d, ("npy",))] == ["a.npy"]
    assert "npy" not in IMG_FORMATS


@pytest.mark.parametrize("bad", [np.zeros((4, 4), np.uint8), np.zeros((4, 4), np.float32), np.zeros((2, 4, 4), np.uint16),
                                 np.zeros(16, np.uint16)])
def test_source_rejects_files_that_are_no_uint16_plane(tmp_path, bad):
    from adaptiveisp_amd.data import ImageFolderSource
    d = _planes(tmp_path, {"good.npy": np.zeros((4, 6), np.uint16), "wrong.npy": bad})
    with pytest.raises(ValueError, match="wrong.npy"):
        ImageFolderSource(d, 32, "cuda:0", data_name="raw", workers=0)


def test_source_construction_errors(tmp_path):
    from adaptiveisp_amd.data import ImageFolderSource
    d = _planes(tmp_path, {"a.npy": np.zeros((4, 6), np.uint16)})
    with pytest.raises(RuntimeError, match="raw"):
        ImageFolderSource(d, 32, "cpu", data_name="raw", workers=0)
    for kw in (dict(add_noise=True), dict(brightness_range=(0.1, 0.5)), dict(noise_level=0.01), dict(use_linear=True),
               dict(sensor="bayer"), dict(raw_gains=(1.0, 2.0))):
        with pytest.raises(ValueError):
            ImageFolderSource(d, 32, "cuda:0", data_name="raw", workers=0, **kw)
    with pytest.raises(FileNotFoundError):
        ImageFolderSource(d, 32, "cpu", data_name="lod", workers=0)             # .npy files are not images
    (tmp_path / "empty").mkdir()
    open(tmp_path / "empty" / "x.png", "wb").close()
    with pytest.raises(ValueError, match="npy"):
        ImageFolderSource(str(tmp_path / "empty"), 32, "cuda:0", data_name="raw", workers=0)   # images are not planes
    src = ImageFolderSource(d, 32, "cuda:0", data_name="raw", workers=0, resize="host", cfa="grbg", raw_bits=10,
                            demosaic="mhc", raw_gains=(1.9, 1.0, 1.6))
    assert len(src) == 1 and (src.white_level, src.black_level) == (1023, 16)
    text = src.describe()
    assert all(s in text for s in ("raw", "GRBG", "10-bit", "black 16", "mhc", "1.9", "1.6")) and "gains" in text
    assert "gains" not in ImageFolderSource(d, 32, "cuda:0", data_name="raw", workers=0).describe()
