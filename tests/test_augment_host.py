"""The training augmentation without a GPU: augment.draw / warp_labels against the reference's fixture
(tests/golden/augment.npz, written by tests/golden/gen_augment.py), the numpy restatement of adaisp_augment_u8
(tests/_augref.py) against properties derived from its formulas and against float64, the planning half of
ImageFolderSource(augment=...), Hyp, the refusals, the command line, the header, exports and descriptor layout."""
import ctypes
import math
import os
import random
import re
import warnings

import numpy as np
import pytest

import _augref as R
from adaptiveisp_amd import _lib
from adaptiveisp_amd.augment import DEFAULTS, Hyp, draw, fixed_inverse, warp_labels
from adaptiveisp_amd.data import ImageFolderSource

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = np.load(os.path.join(ROOT, "tests", "golden", "augment.npz"))
CASES = GOLD["names"].tobytes().decode().split("\n")
KEYS = ("hsv_h", "hsv_s", "hsv_v", "degrees", "translate", "scale", "shear", "perspective", "flipud", "fliplr")    # of hyp_values


def _case(name):
    g = {k.split("/", 1)[1]: GOLD[k] for k in GOLD.files if k.startswith(name + "/")}
    g["hyp"] = dict(zip(KEYS, (float(v) for v in g["hyp_values"])))
    return g


def _rand_u8(seed, h, w):
    return np.random.RandomState(seed).randint(0, 256, size=(h, w, 3)).astype(np.uint8)


def affine(S, degrees, scale, shear, tx=0.5, ty=0.5):
    """random_perspective's M = T S R C for given draws (perspective 0), float64 [3,3]."""
    C, Rm, Sh, T = np.eye(3), np.eye(3), np.eye(3), np.eye(3)
    C[0, 2] = C[1, 2] = -S / 2
    a = degrees * math.pi / 180
    Rm[0, 0] = Rm[1, 1] = scale * math.cos(a)
    Rm[0, 1], Rm[1, 0] = scale * math.sin(a), -scale * math.sin(a)
    Sh[0, 1] = Sh[1, 0] = math.tan(shear * math.pi / 180)
    T[0, 2], T[1, 2] = tx * S, ty * S
    return T @ Sh @ Rm @ C


# ------------------------------------------------------------------------------------------- against the reference
def test_fixture_has_the_cases_the_checks_rest_on():
    assert {f"{k}_{S}" for k in ("rejected", "leaving", "arearatio", "empty", "nohsv") for S in (64, 416)} <= set(CASES)
    assert any(n.startswith("low_") for n in CASES) and any(n.startswith("strong_") for n in CASES)
    assert _case("low_64_0")["hyp"] == DEFAULTS
    for S in (64, 416):
        assert len(_case(f"rejected_{S}")["labels_out"]) < 4 and len(_case(f"empty_{S}")["labels_in"]) == 0
        assert len(_case(f"nohsv_{S}")["luts"]) == 0 and len(_case(f"arearatio_{S}")["labels_out"]) < 25
    assert any(_case(n)["flips"][0] for n in CASES) and any(_case(n)["flips"][1] for n in CASES)


@pytest.mark.parametrize("name", CASES)
def test_draw_and_labels_match_the_reference(name):
    g = _case(name)
    S, seed = int(g["S"]), int(g["seed"])
    d = draw(Hyp(g["hyp"]), random.Random(seed), np.random.RandomState(seed), S)
    assert np.abs(d.M - g["M"]).max() <= 1e-9                  # the same float64 operations; magnitudes <= 1e3
    assert d.s == float(g["s"]) and (bool(d.flipud), bool(d.fliplr)) == tuple(bool(v) for v in g["flips"])
    if len(g["luts"]):
        assert d.luts.dtype == np.uint8 and np.array_equal(d.luts, g["luts"])
    else:
        assert d.luts is None
    got = warp_labels(g["labels_in"], d.M, d.s, d.flipud, d.fliplr, S)
    want = g["labels_out"]
    assert got.shape == want.shape and np.array_equal(got[:, 0], want[:, 0])          # the same rows kept
    if len(want):
        assert np.abs(got[:, 1:] - want[:, 1:]).max() <= 1e-6


def test_no_numpy_draw_without_hsv_gains():
    rs = np.random.RandomState(5)
    before = rs.get_state()[1].copy()
    d = draw(Hyp(hsv_h=0, hsv_s=0, hsv_v=0), random.Random(5), rs, 64)
    assert d.luts is None and np.array_equal(rs.get_state()[1], before)


# ------------------------------------------------------------------------------------ the restatement: derived properties
@pytest.mark.parametrize("fill", [0, 0x727272, 0x0A141E])
def test_identity_reproduces_the_letterboxed_frame(fill):
    for (h, w, top, left, S) in [(37, 64, 13, 0, 64), (1, 1, 5, 7, 16), (20, 9, 3, 11, 50)]:
        img = _rand_u8(h * w, h, w)
        want = R.letterboxed(img, S, top, left, fill)
        assert np.array_equal(R.warp(img, top, left, R.IDENTITY, S, fill), want)
        assert np.array_equal(R.warp(img, top, left, fixed_inverse(np.eye(3), False, False, S), S, fill), want)


def test_flips_mirror_the_frame():
    S, img = 50, _rand_u8(1, 20, 33)
    frame = R.letterboxed(img, S, 7, 4, 0x727272)
    for ud, lr in [(True, False), (False, True), (True, True)]:
        got = R.warp(img, 7, 4, fixed_inverse(np.eye(3), ud, lr, S), S, 0x727272)
        want = frame[::-1] if ud else frame
        want = want[:, ::-1] if lr else want
        assert np.array_equal(got, want)


def test_integer_translation_shifts_and_fills():
    S, img, fill = 64, _rand_u8(2, 30, 40), 0x010203
    frame = R.letterboxed(img, S, 10, 12, fill)
    M = np.eye(3)
    M[0, 2], M[1, 2] = 9, -6                                            # warped (x, y) = frame (x - 9, y + 6)
    got = R.warp(img, 10, 12, fixed_inverse(M, False, False, S), S, fill)
    want = R.letterboxed(np.zeros((0, 0, 3), np.uint8), S, 0, 0, fill)
    want[:S - 6, 9:] = frame[6:, :S - 9]
    assert np.array_equal(got, want)
    M[0, 2] = 3 * S                                                     # past the frame: nothing of it is left
    got = R.warp(img, 10, 12, fixed_inverse(M, False, False, S), S, fill)
    assert np.array_equal(got, R.letterboxed(np.zeros((0, 0, 3), np.uint8), S, 0, 0, fill))


def test_placement_that_does_not_fit_is_all_fill():
    img = _rand_u8(3, 10, 10)
    for top, left in [(60, 0), (0, 55), (-1, 0)]:
        assert np.array_equal(R.warp(img, top, left, R.IDENTITY, 64, 0x727272), np.full((64, 64, 3), 0x72, np.uint8))


def test_warp_of_a_ramp_stays_near_the_float64_bilinear_warp():
    """Slopes of at most 4 levels per pixel per axis, a 10 degree / 0.8 x / 5 degree shear map at S = 64. Bound:
    2 * 4 / 32 (the weights are truncated to 1/32 px in each axis, times the slope) + 0.5 (the final rounding) + 0.01 (the
    map's Q16 rounding: each of fx, fy is off by at most (63 + 63 + 1) * 2^-17 < 0.001 px, times 4 levels, two axes)."""
    S = 64
    yy, xx = np.mgrid[0:S, 0:S]
    img = np.stack([2 * xx + yy + 20, xx + 2 * yy + 5, 3 * xx + 40], axis=-1)
    assert img.max() <= 255 and max(np.abs(np.diff(img, axis=0)).max(), np.abs(np.diff(img, axis=1)).max()) <= 4
    img = img.astype(np.uint8)
    M = affine(S, 10.0, 0.8, 5.0)
    got = R.warp(img, 0, 0, fixed_inverse(M, False, False, S), S, 0).astype(np.float64)
    inv = np.linalg.inv(M)
    u = inv[0, 0] * xx + inv[0, 1] * yy + inv[0, 2]
    v = inv[1, 0] * xx + inv[1, 1] * yy + inv[1, 2]
    inside = (u >= 1) & (u <= S - 3) & (v >= 1) & (v <= S - 3)          # all four taps of both computations in the image
    assert inside.sum() > S * S // 3
    x0, y0 = np.floor(u).astype(int).clip(0, S - 2), np.floor(v).astype(int).clip(0, S - 2)
    a, b = (u - x0)[..., None], (v - y0)[..., None]
    f = img.astype(np.float64)
    want = (1 - a) * (1 - b) * f[y0, x0] + a * (1 - b) * f[y0, x0 + 1] + (1 - a) * b * f[y0 + 1, x0] + a * b * f[y0 + 1, x0 + 1]
    err = np.abs(got - want)[inside].max()
    print("ramp: max |restatement - float64 bilinear| =", err)
    assert err <= 2 * 4 / 32 + 0.5 + 0.01


def test_bgr2hsv_within_one_unit_of_the_rounded_float64_formula():
    vals = np.array(sorted(set([0, 1, 254, 255]) | set(range(5, 250, 4)[:60])))
    assert len(vals) == 64 and {0, 1, 254, 255} <= set(vals.tolist())
    b, g, r = (a.reshape(-1).astype(np.float64) for a in np.meshgrid(vals, vals, vals, indexing="ij"))
    H, S, V = R.bgr2hsv(np.stack([b, g, r], axis=-1))
    v = np.maximum(np.maximum(b, g), r)
    d = v - np.minimum(np.minimum(b, g), r)
    s = np.where(v > 0, 255.0 * d / np.maximum(v, 1), 0.0)
    dd = np.maximum(d, 1)
    deg = np.where(v == r, 60 * (g - b) / dd, np.where(v == g, 120 + 60 * (b - r) / dd, 240 + 60 * (r - g) / dd))
    deg = np.where(deg < 0, deg + 360, deg)
    h = np.where(d > 0, deg / 2, 0.0)
    assert np.array_equal(V, v.astype(np.int64))
    assert np.abs(S - np.rint(s)).max() <= 1
    assert H.min() >= 0 and H.max() < 180 and S.min() >= 0 and S.max() <= 255
    dh = np.abs(H - np.rint(h)) % 180
    dh = np.minimum(dh, 180 - dh)
    assert dh[S > 0].max() <= 1


def test_hsv2bgr_within_one_level_of_the_rounded_float64_formula():
    grid = np.unique(np.concatenate([[0, 1, 254, 255], np.linspace(2, 253, 28).astype(int)]))
    assert len(grid) == 32
    H, S, V = (a.reshape(-1) for a in np.meshgrid(np.arange(180), grid, grid, indexing="ij"))
    got = R.hsv2bgr(H, S, V)
    h, s, v = H / 30.0, S / 255.0, V.astype(np.float64)
    i = np.floor(h).astype(int)
    f = h - i
    p, q, t = v * (1 - s), v * (1 - s * f), v * (1 - s * (1 - f))
    r = np.choose(i, [v, q, p, p, t, v])
    g = np.choose(i, [t, v, v, q, p, p])
    b = np.choose(i, [p, p, t, v, v, q])
    want = np.rint(np.stack([b, g, r], axis=-1))
    assert got.min() >= 0 and got.max() <= 255
    assert np.abs(got - want).max() <= 1


def test_colour_tables_index_by_component():
    lut = np.concatenate([np.arange(256) % 180, np.zeros(256), np.arange(256)]).astype(np.uint8)   # saturation -> 0: grey
    bgr = _rand_u8(4, 8, 8)
    out = R.colour(bgr, lut)
    assert np.array_equal(out, np.repeat(bgr.max(-1, keepdims=True), 3, -1))


# ------------------------------------------------------------------------------------------------------ Hyp
def test_hyp_defaults_dicts_and_yaml(tmp_path):
    assert Hyp().as_dict() == DEFAULTS == Hyp({}).as_dict()
    assert [DEFAULTS[k] for k in ("hsv_h", "hsv_s", "hsv_v", "degrees", "translate", "scale", "shear", "perspective", "flipud",
                                  "fliplr")] == [0.015, 0.7, 0.4, 0, 0.1, 0.5, 0, 0, 0, 0.5]
    y = tmp_path / "hyp.yaml"
    y.write_text("# a YOLO hyper-parameter file\nlr0: 0.01  # initial learning rate\nmomentum: 0.937\nbox: 0.05\nhsv_h: 0.02\n"
                 "hsv_s: 0.6\nhsv_v: 0.3\ndegrees: 5.0\ntranslate: 0.2\nscale: 0.9\nshear: 2.0\nperspective: 0.0\nflipud: 0.1\n"
                 "fliplr: 0.5\nmosaic: 0.0\nmixup: 0.0\ncopy_paste: 0.0\n")
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        h = Hyp(str(y))
    assert h.as_dict() == dict(hsv_h=0.02, hsv_s=0.6, hsv_v=0.3, degrees=5.0, translate=0.2, scale=0.9, shear=2.0, perspective=0.0,
                               flipud=0.1, fliplr=0.5)
    assert Hyp(h) == h and Hyp(dict(degrees=3, lr0=0.01, anchors=3)).degrees == 3.0
    with pytest.raises(ValueError, match="perspective"):
        Hyp(dict(perspective=0.001))
    with pytest.warns(RuntimeWarning, match="mosaic") as rec:
        h = Hyp(dict(mosaic=1.0, degrees=1))
    assert len(rec) == 1 and h.degrees == 1.0
    with pytest.raises(TypeError):
        Hyp(3)


# ------------------------------------------------------------------------------------------ loader (no device), CLI
def _write_pngs(root, sizes, seed=0):
    """PNGs under root/images with YOLO label files under root/labels (image 1 has none)."""
    from PIL import Image
    rs = np.random.RandomState(seed)
    os.makedirs(os.path.join(root, "images"), exist_ok=True)
    os.makedirs(os.path.join(root, "labels"), exist_ok=True)
    for i, (h, w) in enumerate(sizes):
        Image.fromarray(rs.randint(0, 256, size=(h, w, 3)).astype(np.uint8)).save(os.path.join(root, "images", f"im{i:02d}.png"))
        if i != 1:
            with open(os.path.join(root, "labels", f"im{i:02d}.txt"), "w") as f:
                for _ in range(1 + i % 3):
                    cx, cy = rs.uniform(0.3, 0.7, 2)
                    bw, bh = rs.uniform(0.1, 0.4, 2)
                    f.write(f"{rs.randint(80)} {cx:.6f} {cy:.6f} {bw:.6f} {bh:.6f}\n")
    return root


@pytest.fixture(scope="module")
def toy(tmp_path_factory):
    return _write_pngs(str(tmp_path_factory.mktemp("augtoy")), [(48, 64), (64, 40), (20, 30), (64, 64), (33, 17)], seed=1)


def _plans(root, workers, counts=(3, 4, 2, 5), **kw):
    src = ImageFolderSource(root, 64, "cuda:0", seed=3, workers=workers, **kw)      # no device is touched before a batch
    try:
        out = []
        for n in counts:
            items = src._take(n)
            out.append(([it.path for it in items], src._augment_plan(items) if src.augment is not None else None))
        return out, src.rs.get_state()[1].copy(), src.rng.getstate(), list(src.indices)
    finally:
        src.close()


def test_planning_is_the_same_for_every_worker_count_and_leaves_the_other_streams_alone(toy):
    hyp = dict(degrees=10, shear=5, flipud=0.5)
    a, rs_a, rng_a, idx_a = _plans(toy, 0, augment=hyp)
    b, rs_b, rng_b, idx_b = _plans(toy, 4, augment=hyp)
    plain, rs_p, rng_p, idx_p = _plans(toy, 0)
    for (pa, x), (pb, y), (pp, _) in zip(a, b, plain):
        assert pa == pb == pp                                           # the file order of a seed
        assert np.array_equal(x["m"], y["m"]) and np.array_equal(x["lut"], y["lut"]) and np.array_equal(x["luts"], y["luts"])
        assert len(x["labels"]) == len(y["labels"]) and all(np.array_equal(p, q) for p, q in zip(x["labels"], y["labels"]))
        assert x["m"].dtype == np.int64 and x["luts"].shape == (len(pa), 768) and x["lut"].tolist() == list(range(len(pa)))
        for lb, d, m in zip(x["labels"], x["draws"], x["m"]):
            assert lb.dtype == np.float32 and lb.shape[1] == 6 and not lb[:, 0].any()
            assert np.array_equal(m, fixed_inverse(d.M, d.flipud, d.fliplr, 64))
    assert not np.array_equal(a[0][1]["m"][0], a[0][1]["m"][1])          # every image its own draw
    # the metadata stream is untouched; the order stream is where an un-augmented source of the same worker count leaves it
    # (worker threads decode ahead, so it runs ahead of workers=0 with or without augmentation)
    plain4, rs_q, rng_q, idx_q = _plans(toy, 4)
    assert [p for p, _ in plain4] == [p for p, _ in plain]
    assert np.array_equal(rs_a, rs_p) and np.array_equal(rs_b, rs_q) and np.array_equal(rs_p, rs_q)
    assert rng_a == rng_p and idx_a == idx_p and rng_b == rng_q and idx_b == idx_q


def test_planned_labels_are_warp_labels_of_the_loaders(toy):
    from adaptiveisp_amd.val.loader import load_letterboxed
    (paths, plan), = _plans(toy, 0, counts=(5,), augment={})[0]
    kept = 0
    for p, d, got in zip(paths, plan["draws"], plan["labels"]):
        want = warp_labels(load_letterboxed(p, 64)[3], d.M, d.s, d.flipud, d.fliplr, 64)
        assert np.array_equal(got[:, 1:], want.astype(np.float32))
        kept += len(want)
    assert kept > 0


def test_refusals_and_describe(toy, tmp_path):
    with pytest.raises(ValueError, match="raw"):
        ImageFolderSource(toy, 64, "cuda:0", data_name="raw", workers=0, augment={})
    with pytest.raises(ValueError, match="raw"):
        ImageFolderSource(toy, 64, "cpu", data_name="raw", workers=0, augment={})
    with pytest.raises(RuntimeError, match="adaisp_augment_u8"):
        ImageFolderSource(toy, 64, "cpu", workers=0, augment={})
    with pytest.raises(ValueError, match="perspective"):
        ImageFolderSource(toy, 64, "cuda:0", workers=0, augment=dict(perspective=0.1))
    plain = ImageFolderSource(toy, 64, "cpu", workers=0)
    assert plain.augment is None and "augment" not in plain.describe()
    src = ImageFolderSource(toy, 64, "cuda:0", workers=0, augment=Hyp(degrees=5))
    assert src.augment == Hyp(degrees=5) and src.describe().startswith("lod: 5 files, augment (") and "degrees=5" in src.describe()
    y = tmp_path / "h.yaml"
    y.write_text("degrees: 7.5\nlr0: 0.01\n")
    assert ImageFolderSource(toy, 64, "cuda:0", workers=0, augment=str(y)).augment.degrees == 7.5


def test_train_cli_parses_augment_and_hyp(toy, tmp_path, capsys):
    from adaptiveisp_amd.train import parse_args
    a = parse_args(["--data", toy])
    assert a.augment is False and a.hyp is None
    a = parse_args(["--data", toy, "--augment"])
    assert a.augment is True and a.hyp is None
    y = tmp_path / "h.yaml"
    y.write_text("degrees: 7.5\nlr0: 0.01\n")
    a = parse_args(["--data", toy, "--hyp", str(y)])
    assert a.augment is True and a.hyp == Hyp(degrees=7.5)
    for bad in (["--augment"], ["--data", toy, "--data-name", "raw", "--augment"], ["--data", toy, "--hyp", str(tmp_path / "none.yaml")]):
        with pytest.raises(SystemExit) as e:
            parse_args(bad)
        assert e.value.code == 2
    capsys.readouterr()
    from adaptiveisp_amd.val.__main__ import build_parser as val_parser
    assert "--augment" not in val_parser().format_help()                # evaluation does not augment


# ---------------------------------------------------------------------------------------------- C entry and binding
def test_header_exports_and_descriptor_layout():
    hdr = open(os.path.join(ROOT, "include", "adaisp.h")).read()
    assert "int adaisp_augment_u8(" in hdr and "adaisp_augment_desc" in hdr
    assert "adaisp_augment_u8" in _lib.EXPORTS and hasattr(_lib.load(), "adaisp_augment_u8")
    d = _lib.AUGMENT_DESC
    assert d.itemsize == 80
    assert [(n, d.fields[n][1]) for n in ("src_offset", "h", "w", "top", "left", "m", "lut")] == \
        [("src_offset", 0), ("h", 8), ("w", 12), ("top", 16), ("left", 20), ("m", 24), ("lut", 72)]
    m = re.search(r"static_assert\(sizeof\(adaisp_augment_desc\) == (\d+)", open(os.path.join(ROOT, "adaptiveisp_amd", "csrc",
                                                                                            "isp_augment.hip")).read())
    assert m and int(m.group(1)) == d.itemsize


def test_cabi_rejects_bad_arguments_without_launching():
    L = _lib.load()
    p = ctypes.c_void_p(16)
    E, SH = -1, -4

    def call(src=p, src_bytes=64, desc=p, luts=None, n_luts=0, dst=p, B=1, S=8, fill=0):
        return L.adaisp_augment_u8(src, src_bytes, desc, luts, n_luts, dst, B, S, fill, None)

    assert call(src=None) == E and call(desc=None) == E and call(dst=None) == E
    assert call(B=0) == E and call(B=-1) == E and call(S=0) == E
    assert call(n_luts=1) == E and call(luts=p, n_luts=-1) == E                 # tables announced but absent; a negative count
    assert call(fill=0x1000000) == E
    assert call(B=65536) == SH and call(S=32769) == SH
    assert call(src=None, S=32769) == E                                       # EINVAL is reported first


def test_wrapper_checks_come_before_any_device_work():
    import torch
    host = torch.zeros(64, dtype=torch.uint8)
    with pytest.raises(_lib.AdaispError, match="src must be a HIP device tensor"):
        _lib.augment_u8(host, host, None, 8)
    rec = np.zeros(2, _lib.AUGMENT_DESC)
    rec["h"], rec["w"], rec["lut"] = 4, 4, -1
    rec["m"] = R.IDENTITY
    _lib._check_augment_records(rec, 96, 0, 8)
    for field, value, what in [("top", 5, "fit"), ("left", -1, "fit"), ("h", 9, "fit"), ("src_offset", 49, "outside src"),
                               ("lut", 0, "table index"), ("lut", -2, "table index")]:
        bad = rec.copy()
        bad[field][1] = value
        with pytest.raises(_lib.AdaispError, match=what):
            _lib._check_augment_records(bad, 96, 0, 8)
    bad = rec.copy()
    bad["m"][0, 2] = 2 ** 40
    with pytest.raises(_lib.AdaispError, match="wrap"):
        _lib._check_augment_records(bad, 96, 0, 8)
