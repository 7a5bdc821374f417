"""The host half of the raw-capture correction (adaisp_raw_correct), without a GPU: the numpy definition
(tests/_rawfixref.py) against its float64 evaluation and on hand-placed cases, the calibration estimated from dark and flat
frames, the package (header, exports, descriptor layout), the C-ABI's argument checks, RawCalibration and sidecar
validation, the two command lines and the construction of ImageFolderSource with a calibration."""
import ctypes
import json
import os
import re

import numpy as np
import pytest

import _rawfixref as X
from adaptiveisp_amd import _lib
from adaptiveisp_amd.rawcal import (RawCalibration, calibration_from_options, fill_rawfix, level_scale, read_sidecar,
                                    resolve)
from adaptiveisp_amd.rawcal import main as rawcal_main

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BLACK = (60.0, 64.0, 66.5, 71.0)


# ------------------------------------------------------------------------------------------------------------ definition
@pytest.mark.parametrize("shape,grid", [((2, 2), (2, 2)), ((3, 5), (2, 2)), ((37, 53), (5, 7)), ((40, 64), (5, 7)),
                                        ((33, 260), (13, 17))])
def test_definition_is_within_the_derived_bound_of_the_float64_evaluation(shape, grid):
    """0.5 for the final rounding plus twelve fp32 roundings at magnitude <= 2^16, each at most 2^-24 * 2^16 = 2^-8: the
    three level operations round u itself; the nine of the gain (three per interpolation) and the four of the two
    coordinates round numbers near 1, and reach u through a factor below 2^16. Samples whose float64 value leaves
    [0, 65535] are clipped by the definition and left out; they are counted, and are under 5 %."""
    p = X.plane(shape[0], shape[1], sum(shape), hot=0.02 if shape[0] * shape[1] > 100 else 0.0)   # dead samples go under 0
    t = X.table(grid[0], grid[1], 3)
    scale = X.scales(BLACK, 4000.0, 64.0, 4095.0)
    got = X.correct(p, BLACK, scale, 64.0, 40, t).astype(np.float64)
    ex = X.exact(p, BLACK, scale, 64.0, 40, t)
    inside = (ex >= 0) & (ex <= 65535)
    left_out = int((~inside).sum())
    print(f"{shape}: {left_out} of {p.size} samples left out, max error {np.abs(got - ex)[inside].max():.6f}")
    assert left_out < 0.05 * p.size
    assert np.abs(got - ex)[inside].max() <= 0.5 + 12 * 2.0 ** -8


def test_identity_configuration_returns_the_plane():
    p = np.random.RandomState(0).randint(0, 65536, size=(37, 53)).astype(np.uint16)
    assert np.array_equal(X.correct(p), p)
    assert np.array_equal(X.correct(p, (64.0,) * 4, (1.0,) * 4, 64.0), p)
    assert np.array_equal(X.correct(p, (66.5,) * 4, (1.0,) * 4, 66.5, dpc=-1, table=None), p)


def test_defect_rule_on_hand_placed_cases():
    cases = X.defect_cases()
    assert [c[1] for c in cases] == [50, 50, 50, 50, 0, -1]
    for p, dpc, want in cases:
        assert np.array_equal(X.correct(p, dpc=dpc), want), dpc
    hot, _, base = cases[0]
    assert len(X.SITES) == 12 and (hot != base).sum() == 12           # every position at a corner, an edge, inside
    pos = {(2 * (y & 1) + (x & 1), kind) for (y, x), kind in zip(X.SITES, ["corner"] * 4 + ["edge"] * 4 + ["inside"] * 4)}
    assert len(pos) == 12
    pair = cases[3][0]
    assert pair[4, 4] == pair[4, 6] == 3000 and np.array_equal(X.correct(pair, dpc=50), pair)
    assert X.correct(pair, dpc=50)[4, 4] == 3000                      # corrected one at a time it would have gone


def test_ties_round_to_even_and_the_result_is_clipped():
    p, c, want = X.tie_case()
    assert np.array_equal(X.correct(p, **c), want) and want[0].tolist() == [0, 2, 2, 4, 4, 6]
    p, c, want = X.clip_case()
    assert np.array_equal(X.correct(p, **c), want) and want.min() == 0 and want.max() == 65535
    assert X.correct(p, black=(np.nan,) * 4).max() == 0               # NaN gives 0


# ------------------------------------------------------------------------------------------------------------ from_frames
GRID = (25, 33)


def _sensor(H=120, W=160):
    yy, xx = np.mgrid[0:H, 0:W]
    k = 2 * (yy & 1) + (xx & 1)
    r2 = (((yy - (H - 1) / 2) / ((H - 1) / 2)) ** 2 + ((xx - (W - 1) / 2) / ((W - 1) / 2)) ** 2) / 2
    black = np.array([60.0, 64.0, 66.0, 71.0])
    flat = np.rint(black[k] + 3000.0 * (1.0 - 0.5 * r2)).astype(np.uint16)      # to half at the corners
    return k, black, black[k].astype(np.uint16), flat


def test_from_frames_round_trip():
    """Noise-free, 120 x 160, four black levels, a radial fall-off to half at the corners. The issue's 13 x 17 grid does
    not meet the cap in float64 (the estimator's own error: non-flatness 0.0785 against a cap of 0.0585; the window
    means are biased where the fall-off is steep and the window is clipped), so, as the issue rules, the grid is enlarged,
    not the cap: 25 x 33 gives 0.0299 in float64."""
    k, black, dark, flat = _sensor()
    cal = RawCalibration.from_frames([dark, dark], [flat, flat], "RGGB", grid=GRID, white=4095)
    assert np.abs(cal.black - black).max() <= 1e-9
    assert cal.shading.dtype == np.float32 and cal.shading.shape == (4,) + GRID
    assert cal.shading.min() >= 1.0 and cal.shading.max() <= 8.0 and cal.shading.max() > 1.8
    got = X.correct(flat, cal.black, (1.0,) * 4, 0.0, -1, cal.shading).astype(np.float64)
    ex = X.exact(flat, cal.black, (1.0,) * 4, 0.0, -1, cal.shading)
    for pos in range(4):
        m = k == pos
        nf = lambda a: (a[m].max() - a[m].min()) / a[m].mean()
        before = nf(flat.astype(np.float64))
        print(f"position {pos}: flat {before:.4f}, float64 {nf(ex):.4f}, fp32 {nf(got):.4f}")
        assert nf(ex) <= 0.6 * before / 10                            # the float64 evaluation alone, with room
        assert nf(got) <= nf(ex) + 2.0 / got[m].mean()                # one count of rounding each way
        assert nf(got) < before / 10


def test_from_frames_clamps_and_validates(tmp_path):
    k, black, dark, flat = _sensor(24, 32)
    dim = flat.copy()
    dim[:6, :8] = dark[:6, :8] + 1                                    # a corner 3000 times darker than the centre
    cal = RawCalibration.from_frames([dark], [dim], "GRBG", grid=(5, 5), max_gain=4.0, white=4095, dpc=12)
    assert cal.shading.max() == 4.0 and cal.shading.min() == 1.0 and (cal.cfa, cal.dpc, cal.white) == ("GRBG", 12, 4095.0)
    for bad in (dict(dark=[], flat=[flat]), dict(dark=[dark], flat=[flat[:-2]]), dict(dark=[dark.astype(np.int32)], flat=[flat]),
                dict(dark=[dark], flat=[flat], grid=(1, 5)), dict(dark=[dark], flat=[flat], max_gain=0.5)):
        with pytest.raises(ValueError):
            RawCalibration.from_frames(**bad)
    for name, frames in (("dark", [dark, dark]), ("flat", [flat])):
        os.makedirs(tmp_path / name)
        for i, f in enumerate(frames):
            np.save(tmp_path / name / f"{i}.npy", f)
    out = tmp_path / "cal.npz"
    assert rawcal_main(["--dark", str(tmp_path / "dark"), "--flat", str(tmp_path / "flat"), "--cfa", "RGGB", "--white", "4095",
                        "--grid", "5", "7", "--dpc", "40", "--out", str(out)]) == 0
    cal = RawCalibration.load(out)
    ref = RawCalibration.from_frames([dark, dark], [flat], "RGGB", grid=(5, 7), white=4095, dpc=40)
    assert np.array_equal(cal.shading, ref.shading) and np.array_equal(cal.black, ref.black) and cal.dpc == 40
    with pytest.raises(SystemExit) as e:
        rawcal_main(["--dark", str(tmp_path), "--flat", str(tmp_path / "flat"), "--white", "4095", "--out", str(out)])
    assert e.value.code == 2


# ------------------------------------------------------------------------------------------------------------ package
def _header():
    text = open(os.path.join(ROOT, "include", "adaisp.h")).read()
    return text, re.sub(r"/\*.*?\*/", "", text, flags=re.S)


def test_header_library_and_descriptor():
    text, code = _header()
    assert re.search(r"\bint\s+adaisp_raw_correct\s*\(", code)
    assert "adaisp_raw_correct" in _lib.EXPORTS
    L = _lib.load()
    assert hasattr(L, "adaisp_raw_correct")
    assert re.search(r"#define\s+ADAISP_ABI_VERSION\s+9\b", text) and L.adaisp_abi_version() == 9 == _lib.ABI_VERSION

    class Desc(ctypes.Structure):                                     # the header's fields, in its order
        _fields_ = [("src_offset", ctypes.c_int64), ("dst_offset", ctypes.c_int64), ("src_h", ctypes.c_int32),
                    ("src_w", ctypes.c_int32), ("grid", ctypes.c_int64), ("grid_h", ctypes.c_int32),
                    ("grid_w", ctypes.c_int32), ("step_y", ctypes.c_float), ("step_x", ctypes.c_float),
                    ("black", ctypes.c_float * 4), ("scale", ctypes.c_float * 4), ("black_out", ctypes.c_float),
                    ("dpc", ctypes.c_int32), ("reserved", ctypes.c_int32 * 2)]
    body = re.search(r"typedef struct adaisp_rawfix_desc \{(.*?)\} adaisp_rawfix_desc;", code, flags=re.S).group(1)
    names = re.findall(r"(\w+)(?:\[\d+\])?\s*[,;]", body)
    assert names == [f[0] for f in Desc._fields_] == list(_lib.RAWFIX_DESC.names)
    assert _lib.RAWFIX_DESC.itemsize == ctypes.sizeof(Desc) == 96
    for name, _ in Desc._fields_:
        assert _lib.RAWFIX_DESC.fields[name][1] == getattr(Desc, name).offset, name


def test_argument_checks_without_gpu():
    L = _lib.load()
    a, b = (ctypes.c_float * 64)(), (ctypes.c_float * 64)()
    pa, pb = ctypes.cast(a, ctypes.c_void_p), ctypes.cast(b, ctypes.c_void_p)

    def call(src=pa, dst=pb, desc=pa, gains=pa, B=1, src_bytes=128, dst_bytes=128, words=16):
        return L.adaisp_raw_correct(src, src_bytes, dst, dst_bytes, desc, gains, words, B, None)

    for null in ("src", "dst", "desc", "gains"):
        assert call(**{null: None}) == -1, null
    assert call(gains=None, words=0, B=0) == 0                        # no table at all is fine
    assert call(src=ctypes.c_void_p(pa.value + 1)) == -1 and call(dst=ctypes.c_void_p(pb.value + 1)) == -1
    assert call(B=-1) == -1
    assert call(dst=pa) == -3                                         # in place
    assert call(dst=ctypes.c_void_p(pa.value + 126)) == -3 and call(src=ctypes.c_void_p(pb.value + 126)) == -3
    lo, hi = sorted((pa.value, pb.value))
    if hi - lo >= 256:                                                # touching ranges do not overlap
        assert call(src=ctypes.c_void_p(lo), dst=ctypes.c_void_p(lo + 128), B=0) == 0
    assert call(B=65536) == -4
    assert call(B=0) == 0                                             # nothing to do, nothing launched


def test_fill_rawfix_and_level_scale():
    rec = np.zeros(2, _lib.RAWFIX_DESC)
    fill_rawfix(rec[0], (37, 53), 16, 4000, BLACK, level_scale(BLACK, 4000, 64, 4095), 64, 40, (8, 5, 7))
    fill_rawfix(rec[1], (2, 2), 0, 0, (0,) * 4, (1,) * 4, 0, None, None)
    assert (rec[0]["src_offset"], rec[0]["dst_offset"], rec[0]["src_h"], rec[0]["src_w"]) == (16, 4000, 37, 53)
    assert (rec[0]["grid"], rec[0]["grid_h"], rec[0]["grid_w"], rec[0]["dpc"]) == (8, 5, 7, 40)
    assert (rec[0]["step_y"], rec[0]["step_x"]) == X.steps((37, 53), (5, 7)) == (np.float32(4 / 36), np.float32(6 / 52))
    assert np.array_equal(rec[0]["scale"], X.scales(BLACK, 4000, 64, 4095)) and rec[0]["black"].tolist() == list(BLACK)
    assert (rec[1]["grid"], rec[1]["dpc"]) == (-1, -1) and rec[1]["scale"].tolist() == [1.0] * 4
    assert not rec["reserved"].any()


# ------------------------------------------------------------------------------------------------------------ calibration
def test_calibration_validation_names_the_field():
    t = X.table(3, 4)
    ok = RawCalibration(BLACK, 4000, t, 40, "grbg")
    assert ok.cfa == "GRBG" and ok.black.tolist() == list(BLACK) and ok.shading.dtype == np.float32 and ok.dpc == 40
    assert RawCalibration(64, 4095).black.tolist() == [64.0] * 4
    assert RawCalibration(None, None, dpc=0).black is None
    bad = [("black", dict(black=(1, 2, 3))), ("black", dict(black="64")), ("black", dict(black=(1, 2, 3, np.nan))),
           ("black", dict(black=-1)), ("white", dict(white=60)), ("white", dict(white=np.inf)), ("white", dict(white=(1, 2))),
           ("shading", dict(shading=t[:3])), ("shading", dict(shading=t[:, :1])), ("shading", dict(shading=t * 0)),
           ("shading", dict(shading=np.where(t > 1.2, np.nan, t))), ("shading", dict(shading=t[0])),
           ("dpc", dict(dpc=-1)), ("dpc", dict(dpc=1.5)), ("dpc", dict(dpc=True)), ("cfa", dict(cfa="RGBG")),
           ("cfa", dict(cfa=None))]
    for field, kw in bad:
        with pytest.raises(ValueError, match="^" + field):
            RawCalibration(**{**dict(black=BLACK, white=4000), **kw})


def test_calibration_save_load_round_trip(tmp_path):
    t = X.table(5, 7, 2)
    cal = RawCalibration(BLACK, 4000, t, 40, "GBRG")
    cal.save(tmp_path / "cal.npz")
    with np.load(tmp_path / "cal.npz", allow_pickle=False) as z:
        assert sorted(z.files) == ["black", "cfa", "dpc", "shading", "white"]
    back = RawCalibration.load(tmp_path / "cal.npz")
    assert np.array_equal(back.black, cal.black) and back.white == 4000.0 and np.array_equal(back.shading, t)
    assert (back.dpc, back.cfa) == (40, "GBRG") and "cal.npz" in back.describe() and "shading 5x7" in back.describe()
    RawCalibration(None, None, dpc=7).save(tmp_path / "dpc.npz")
    only = RawCalibration.load(tmp_path / "dpc.npz")
    assert only.black is None and only.white is None and only.shading is None and only.dpc == 7
    np.savez(tmp_path / "other.npz", cfa=np.array("RGGB"), weights=np.zeros(3))
    open(tmp_path / "junk.npz", "wb").write(b"not a zip")
    for name in ("other.npz", "junk.npz", "missing.npz"):
        with pytest.raises(ValueError, match=name):
            RawCalibration.load(tmp_path / name)
    assert calibration_from_options(None, None, "RGGB") is None
    assert calibration_from_options(None, 9, "BGGR").dpc == 9 and calibration_from_options(None, 9, "BGGR").cfa == "BGGR"
    assert calibration_from_options(str(tmp_path / "cal.npz"), None, "GBRG").dpc == 40
    over = calibration_from_options(str(tmp_path / "cal.npz"), 5, "GBRG")
    assert over.dpc == 5 and np.array_equal(over.shading, t) and over.white == 4000.0


def test_sidecars(tmp_path):
    def side(doc, raw=None):
        with open(tmp_path / "cap.json", "w") as f:
            f.write(raw if raw is not None else json.dumps(doc))
        return read_sidecar(str(tmp_path / "cap.npy"))

    assert read_sidecar(str(tmp_path / "none.npy")) is None
    assert side({}) == {}
    assert side({"black_level": 64})["black"].tolist() == [64.0] * 4                    # one level
    assert side({"black_level": [60, 64, 66.5, 71]})["black"].tolist() == list(BLACK)   # four
    assert side({"white_level": 16383}) == {"white": 16383.0}
    assert side({"gains": [1.9, 1, 1.6], "iso": 6400}) == {"gains": (1.9, 1.0, 1.6)}
    for doc in ({"black_level": [1, 2]}, {"black_level": "64"}, {"black_level": -3}, {"white_level": [4095]},
                {"white_level": 0}, {"gains": [1, 2]}, {"gains": [1, 2, "x"]}, {"gains": 2.0}, [1, 2, 3]):
        with pytest.raises(ValueError, match="cap.json"):
            side(doc)
    with pytest.raises(ValueError, match="cap.json"):
        side(None, raw="{black_level: 64")
    cal = RawCalibration(BLACK, 4000)
    assert resolve(None, None, 64, 4095)[0].tolist() == [64.0] * 4 and resolve(None, None, 64, 4095)[1] == 4095.0
    b, w = resolve(cal, None, 64, 4095)
    assert b.tolist() == list(BLACK) and w == 4000.0
    b, w = resolve(cal, {"white": 16383.0}, 64, 4095)
    assert b.tolist() == list(BLACK) and w == 16383.0
    b, w = resolve(cal, {"black": np.full(4, 256.0)}, 64, 4095)
    assert b.tolist() == [256.0] * 4 and w == 4000.0
    with pytest.raises(ValueError, match="somewhere"):
        resolve(cal, {"white": 50.0}, 64, 4095, where="somewhere")


# ------------------------------------------------------------------------------------------------------------ CLIs
def test_cli_parsing(capsys):
    from adaptiveisp_amd import train
    from adaptiveisp_amd.val.__main__ import parse_args as val_args
    base = ["--isp-ckpt", "x.pth", "--data", "planes"]
    a = val_args(base + ["--data-name", "raw", "--raw-cal", "cal.npz", "--raw-dpc", "30", "--raw-meta"])
    assert (a.raw_cal, a.raw_dpc, a.raw_meta) == ("cal.npz", 30, True)
    a = val_args(base + ["--data-name", "raw"])
    assert (a.raw_cal, a.raw_dpc, a.raw_meta) == (None, None, False)
    t = train.parse_args(["--data", "planes", "--data-name", "raw", "--raw-dpc", "0"])
    assert (t.raw_cal, t.raw_dpc, t.raw_meta) == (None, 0, False)
    for parse, argv in ((val_args, base), (train.parse_args, ["--data", "planes"])):
        for bad in (["--raw-cal", "cal.npz"], ["--raw-dpc", "30"], ["--raw-meta"], ["--data-name", "coco", "--raw-meta"],
                    ["--data-name", "raw", "--raw-dpc", "-1"], ["--data-name", "raw", "--raw-dpc", "x"]):
            with pytest.raises(SystemExit) as e:
                parse(argv + bad)
            assert e.value.code == 2, bad
    capsys.readouterr()


# ------------------------------------------------------------------------------------------------------------ source
def test_source_construction(tmp_path):
    from adaptiveisp_amd.data import ImageFolderSource
    d = tmp_path / "images"
    d.mkdir()
    np.save(d / "a.npy", np.zeros((4, 6), np.uint16))
    np.save(d / "b.npy", np.zeros((6, 4), np.uint16))
    cal = RawCalibration(BLACK, 4000, X.table(3, 4), 40)
    kw = dict(data_name="raw", workers=0)
    for other in ("lod", "coco"):
        with pytest.raises(ValueError, match="raw"):
            ImageFolderSource(str(d), 32, "cuda:0", data_name=other, workers=0, raw_meta=True)
        with pytest.raises(ValueError, match="raw"):
            ImageFolderSource(str(d), 32, "cuda:0", data_name=other, workers=0, raw_calibration=cal)
    with pytest.raises(ValueError, match="GRBG"):
        ImageFolderSource(str(d), 32, "cuda:0", cfa="GRBG", raw_calibration=cal, **kw)
    with pytest.raises(ValueError):
        ImageFolderSource(str(d), 32, "cuda:0", raw_calibration=3, **kw)
    src = ImageFolderSource(str(d), 32, "cuda:0", raw_calibration=cal, raw_meta=True, **kw)
    assert src._rawfix and all(s in src.describe() for s in ("calibration", "shading 3x4", "dpc 40", "0 sidecars"))
    plain = ImageFolderSource(str(d), 32, "cuda:0", **kw)
    assert not plain._rawfix and "calibration" not in plain.describe() and "sidecars" not in plain.describe()
    assert not ImageFolderSource(str(d), 32, "cuda:0", raw_meta=True, **kw)._rawfix     # no sidecar: nothing in play
    json.dump({"gains": [2, 1, 1.5]}, open(d / "a.json", "w"))
    src = ImageFolderSource(str(d), 32, "cuda:0", raw_meta=True, **kw)
    assert src._rawfix and "1 sidecars" in src.describe()
    assert not ImageFolderSource(str(d), 32, "cuda:0", **kw)._rawfix                   # sidecars are opt-in
    cal.save(tmp_path / "cal.npz")
    assert "cal.npz" in ImageFolderSource(str(d), 32, "cuda:0", raw_calibration=str(tmp_path / "cal.npz"), **kw).describe()
    open(d / "b.json", "w").write("{")
    with pytest.raises(ValueError, match="b.json"):
        ImageFolderSource(str(d), 32, "cuda:0", raw_meta=True, **kw)
    json.dump({"white_level": 50}, open(d / "b.json", "w"))                             # under the black level
    with pytest.raises(ValueError, match="b.npy"):
        ImageFolderSource(str(d), 32, "cuda:0", raw_meta=True, **kw)
