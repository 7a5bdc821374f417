"""Mosaic and mixup without a GPU: augment.draw_mosaic / mosaic_tiles / mosaic_boxes against the reference's fixture
(tests/golden/mosaic_aug.npz, written by tests/golden/gen_mosaic.py from the reference's own load_mosaic), the numpy
restatement of adaisp_mosaic_u8 (tests/_mosaicref.py) assembling the reference's canvas from the tile records, the planning
half of ImageFolderSource(mosaic=...), the refusals of the loader, the wrapper and the command line, the header and layout."""
import os
import random
import re
import warnings

import numpy as np
import pytest

import _augref as A
import _mosaicref as R
from adaptiveisp_amd import _lib
from adaptiveisp_amd.augment import (Hyp, draw, draw_mosaic, fill_mosaic_layer, fill_single_layer, finish_labels, fixed_inverse,
                                     mix_q16, mosaic_boxes, mosaic_tiles, warp_labels)
from adaptiveisp_amd.data import ImageFolderSource
from test_augment_host import _write_pngs

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = np.load(os.path.join(ROOT, "tests", "golden", "mosaic_aug.npz"))
NAMES = GOLD["names"].tobytes().decode().split("\n")
CASES = [n for n in NAMES if not n.startswith("mixup_")]
MIXUPS = [n for n in NAMES if n.startswith("mixup_")]
KEYS = ("hsv_h", "hsv_s", "hsv_v", "degrees", "translate", "scale", "shear", "perspective", "flipud", "fliplr")    # of hyp_values
GREY = 0x727272                                   # the reference's canvas colour, 114


def case(name):
    g = {k.split("/", 1)[1]: GOLD[k] for k in GOLD.files if k.startswith(name + "/")}
    if "hyp_values" in g:
        g["hyp"] = dict(zip(KEYS, (float(v) for v in g["hyp_values"])))
        rs = np.random.RandomState(int(g["seed"]))                       # gen_mosaic.py's tiles_of
        g["tiles"] = [rs.randint(0, 256, size=(int(h), int(w), 3)).astype(np.uint8) for h, w in g["sizes"]]
        g["labels"] = [g["labels_in"][g["labels_in"][:, 0] == i, 1:] for i in range(len(g["sizes"]))]
    return g


def records_of(g, m, fill=GREY, gap=0):
    """One one-layer record of the case's four tiles, and the bytes they point into (`gap` filler bytes before each)."""
    S = int(g["S"])
    order = [int(i) for i in g["order"]]
    sizes = [tuple(int(v) for v in g["sizes"][i]) for i in order]
    rec = np.zeros(1, _lib.MOSAIC_DESC)
    rec["n_layers"], rec["lut"], rec["mix"] = 1, -1, 65536
    lay = rec[0]["layer"][0]
    fill_mosaic_layer(lay, m, sizes, mosaic_tiles(sizes, tuple(int(v) for v in g["centre"]), S))
    lay["fill"] = fill
    chunks, off = [], 0
    for k, i in enumerate(order):
        lay["tile"][k]["src_offset"] = off + gap
        chunks += [np.full(gap, 77, np.uint8), g["tiles"][i].reshape(-1)]
        off += gap + g["tiles"][i].size
    return rec, np.concatenate(chunks)


def crop_map(S):
    """Scale 1, translation (S / 2, S / 2): the output is the canvas's centre S x S."""
    return (65536, 0, S // 2 * 65536, 0, 65536, S // 2 * 65536)


# ------------------------------------------------------------------------------------------- against the reference
def test_fixture_has_the_cases_the_checks_rest_on():
    for S in (32, 64):
        assert {f"{k}_{S}" for k in ("small", "large", "mixed", "empty", "leaving", "rejected")} <= set(CASES)
        g = case(f"small_{S}")
        assert (g["canvas"][S // 2:3 * S // 2, S // 2:3 * S // 2] == 114).all(axis=-1).any()      # fill shows in the crop
        g = case(f"large_{S}")
        assert not (g["canvas"][S // 2:3 * S // 2, S // 2:3 * S // 2] == 114).all(axis=-1).any()  # tiles cropped: none shows
        sizes = case(f"mixed_{S}")["sizes"]
        assert (sizes[:, 0] > sizes[:, 1]).any() and (sizes[:, 0] < sizes[:, 1]).any()            # portrait and landscape
        assert len(case(f"empty_{S}")["labels_in"]) == 0 and len(case(f"empty_{S}")["labels_out"]) == 0
        assert 0 < len(case(f"leaving_{S}")["labels_out"]) < 16 and len(case(f"rejected_{S}")["labels_out"]) < 12
    assert len(MIXUPS) == 4
    assert os.path.getsize(os.path.join(ROOT, "tests", "golden", "mosaic_aug.npz")) < 400 * 1024


@pytest.mark.parametrize("name", CASES)
def test_draw_tiles_and_labels_match_the_reference(name):
    g = case(name)
    S, seed, n = int(g["S"]), int(g["seed"]), len(g["sizes"])
    nprs = np.random.RandomState(seed)
    before = nprs.get_state()[1].copy()
    d = draw_mosaic(Hyp(g["hyp"]), random.Random(seed), nprs, S, n, int(g["index"]))
    assert np.array_equal(nprs.get_state()[1], before)                 # load_mosaic draws from `random` alone
    assert list(d.indices) == g["order"].tolist() and list(d.centre) == g["centre"].tolist()
    assert np.abs(d.M - g["M"]).max() <= 1e-12 and abs(d.s - float(g["s"])) <= 1e-12
    sizes = [tuple(int(v) for v in g["sizes"][i]) for i in d.indices]
    tiles = mosaic_tiles(sizes, d.centre, S)
    assert tiles.dtype == np.int64 and tiles.shape == (4, 6)
    boxes = mosaic_boxes([g["labels"][i] for i in d.indices], sizes, tiles, d.M, d.s, S)
    assert boxes.shape == g["labels_warped"].shape and boxes.dtype == np.float64
    if len(boxes):
        assert np.array_equal(boxes[:, 0], g["labels_warped"][:, 0]) and np.abs(boxes - g["labels_warped"]).max() <= 1e-12
    out = finish_labels(boxes, S, False, False)
    assert out.shape == g["labels_out"].shape and (not len(out) or np.abs(out - g["labels_out"]).max() <= 1e-12)
    flipped = finish_labels(boxes, S, True, True)
    assert np.array_equal(flipped[:, [0, 3, 4]], out[:, [0, 3, 4]]) and np.array_equal(flipped[:, 1:3], 1 - out[:, 1:3])


@pytest.mark.parametrize("name", MIXUPS)
def test_mixup_labels_and_ratio_match_the_reference(name):
    g = case(name)
    S, seed = int(g["S"]), int(g["seed"])
    r = np.random.RandomState(seed).beta(32.0, 32.0)
    assert r == float(g["r"]) and mix_q16(r) == int(np.rint(65536 * float(g["r"]))) and 0 < mix_q16(r) < 65536
    first, second = g["of"].tobytes().decode().split("\n")
    rows = np.concatenate([case(first)["labels_warped"], case(second)["labels_warped"]])
    out = finish_labels(rows, S, False, False)
    assert out.shape == g["labels_out"].shape and np.abs(out - g["labels_out"]).max() <= 1e-12


@pytest.mark.parametrize("name", CASES)
def test_restatement_assembles_the_reference_canvas_from_the_tile_records(name):
    g = case(name)
    S = int(g["S"])
    rec, src = records_of(g, crop_map(S), gap=3)
    _lib._check_mosaic_records(rec, src.size, 0)
    assert np.array_equal(R.mosaic(src, rec[0], S), g["canvas"][S // 2:3 * S // 2, S // 2:3 * S // 2])
    # and the four S x S quarters of the whole canvas, through translations alone
    for oy in (0, S):
        for ox in (0, S):
            rec[0]["layer"][0]["m"] = (65536, 0, ox * 65536, 0, 65536, oy * 65536)
            assert np.array_equal(R.mosaic(src, rec[0], S), g["canvas"][oy:oy + S, ox:ox + S])


def test_restatement_one_layer_one_tile_is_the_augment_restatement():
    S, rs = 50, np.random.RandomState(4)
    img = rs.randint(0, 256, size=(31, 44, 3)).astype(np.uint8)
    d = draw(Hyp(degrees=10, shear=5, flipud=0.5, hsv_h=0.5), random.Random(4), rs, S)
    m = fixed_inverse(d.M, True, True, S)
    rec = np.zeros(1, _lib.MOSAIC_DESC)
    rec["n_layers"], rec["lut"] = 1, 0
    lay = rec[0]["layer"][0]
    fill_single_layer(lay, m, 31, 44, 9, 3)
    lay["fill"], lay["tile"][0]["src_offset"] = 0x302010, 5
    src = np.concatenate([np.full(5, 9, np.uint8), img.reshape(-1)])
    luts = d.luts.reshape(1, 768)
    assert np.array_equal(R.mosaic(src, rec[0], S, luts), A.augment(img, 9, 3, m.tolist(), S, 0x302010, luts[0]))


def test_restatement_seams_blend_and_absent_tiles_are_fill():
    """Half a pixel right and down at scale 1: every output pixel is the mean of four canvas pixels, so a pixel on a seam
    has taps in two tiles (or a tile and the fill) and is their rounded mean."""
    g = case("small_32")
    S = 32
    rec, src = records_of(g, (65536, 0, S // 2 * 65536 + 32768, 0, 65536, S // 2 * 65536 + 32768))
    c = g["canvas"].astype(np.int64)
    y, x = np.mgrid[S // 2:3 * S // 2, S // 2:3 * S // 2]
    want = (256 * (c[y, x] + c[y, x + 1] + c[y + 1, x] + c[y + 1, x + 1]) + 512) >> 10
    assert np.array_equal(R.mosaic(src, rec[0], S), want.astype(np.uint8))
    short = src[:-1]                              # the last tile's bytes no longer lie inside src: it is absent, the rest stays
    last = rec[0]["layer"][0]["tile"][3]
    assert not R.tile_present(last, short.size) and all(R.tile_present(rec[0]["layer"][0]["tile"][k], short.size) for k in range(3))
    blank = g["canvas"].copy()
    blank[int(last["y0"]):int(last["y1"]), int(last["x0"]):int(last["x1"])] = 114
    rec[0]["layer"][0]["m"] = crop_map(S)
    assert np.array_equal(R.mosaic(short, rec[0], S), blank[S // 2:3 * S // 2, S // 2:3 * S // 2])


@pytest.mark.parametrize("name", MIXUPS)
def test_restatement_mix_tracks_the_reference_mixup(name):
    """Weight error <= 2^-17 and 255 * 2^-17 << 1: floor against floor differs by at most one step."""
    g = case(name)
    S, seed = int(g["S"]), int(g["seed"])
    rs = np.random.RandomState(seed)
    a, b = (rs.randint(0, 256, size=(S, S, 3)).astype(np.int64) for _ in range(2))
    mix = mix_q16(float(g["r"]))
    got = (mix * a + (65536 - mix) * b) >> 16
    assert np.abs(got - g["mixed"].astype(np.int64)).max() <= 1


# ------------------------------------------------------------------------------------------------------- the loader
SIZES = [(48, 64), (64, 40), (20, 30), (64, 64), (100, 80), (33, 17), (150, 200)]


@pytest.fixture(scope="module")
def toy(tmp_path_factory):
    return _write_pngs(str(tmp_path_factory.mktemp("mosaictoy")), SIZES, seed=2)


def _plans(root, workers, counts=(3, 4, 2), **kw):
    src = ImageFolderSource(root, 64, "cuda:0", seed=3, workers=workers, augment=dict(degrees=10, shear=5, flipud=0.5), **kw)
    try:
        out = []
        for n in counts:
            samples = src._take_samples(n)
            out.append((samples, src._mosaic_plan(samples)))
        return out, src.rs.get_state()[1].copy(), src.describe()
    finally:
        src.close()


def test_two_sources_with_the_same_seed_draw_identically(toy):
    a, rs_a, text = _plans(toy, 0, mosaic=0.7, mixup=0.5)
    b, rs_b, _ = _plans(toy, 3, mosaic=0.7, mixup=0.5)
    c, _, _ = _plans(toy, 0, mosaic=0.7, mixup=0.5, resize="device")
    assert text.endswith(", mosaic 0.7, mixup 0.5") and np.array_equal(rs_a, rs_b)
    kinds = set()
    for (sa, pa), (sb, pb), (sc, pc) in zip(a, b, c):
        assert pa["records"].tobytes() == pb["records"].tobytes() == pc["records"].tobytes()
        assert np.array_equal(pa["luts"], pb["luts"]) and pa["n_layers"] == pb["n_layers"] and pa["slots"] == pb["slots"]
        assert all(np.array_equal(p, q) and np.array_equal(p, r) for p, q, r in zip(pa["labels"], pb["labels"], pc["labels"]))
        assert [it.path for it in pa["items"]] == [it.path for it in pb["items"]] == [it.path for it in pc["items"]]
        for s, rec, lb in zip(sa, pa["records"], pa["labels"]):
            kinds.add(len(s.plan.mosaics))
            assert len(s.items) == max(1, 4 * len(s.plan.mosaics)) and rec["n_layers"] == max(1, len(s.plan.mosaics))
            assert (s.plan.r is None) == (len(s.plan.mosaics) < 2) and lb.dtype == np.float32 and lb.shape[1] == 6
            assert rec["mix"] == (65536 if s.plan.r is None else mix_q16(s.plan.r))
            assert s.plan.mosaics == () or s.plan.mosaics[0].indices.count(s.plan.index) >= 1
        _lib._check_mosaic_records(pa["records"], 1 << 40, len(pa["luts"]))
    assert kinds == {0, 1, 2}                     # single images, mosaics and mixed pairs in these nine


def test_planned_records_and_labels_are_those_of_the_draws(toy):
    """A twin pair of generators, drawn in the documented order, gives the plan's maps, tiles and labels."""
    from adaptiveisp_amd.augment import draw_colour_flips
    from adaptiveisp_amd.data import AUGMENT_SEED
    from adaptiveisp_amd.val.loader import _label_path, load_image, load_letterboxed, read_labels
    (samples, plan), = _plans(toy, 0, counts=(6,), mosaic=0.6, mixup=0.5)[0]
    files = sorted(os.path.join(toy, "images", f) for f in os.listdir(os.path.join(toy, "images")))
    rng, nprs, hyp, S = random.Random(3000 + AUGMENT_SEED), np.random.RandomState(3000 + AUGMENT_SEED), Hyp(degrees=10, shear=5, flipud=0.5), 64
    for b, s in enumerate(samples):
        rec = plan["records"][b]
        assert s.plan.index == b                                        # the first pass is in file order
        if not rng.random() < 0.6:
            d = draw(hyp, rng, nprs, S)
            im, (top, left), _, lb, _ = load_letterboxed(files[b], S)
            assert s.plan.mosaics == () and np.array_equal(rec["layer"][0]["m"], fixed_inverse(d.M, d.flipud, d.fliplr, S))
            t = rec["layer"][0]["tile"][0]
            assert (t["h"], t["w"], t["x0"], t["y0"], t["dx"], t["dy"]) == (*im.shape[:2], left, top, left, top)
            assert np.array_equal(plan["labels"][b][:, 1:], warp_labels(lb, d.M, d.s, d.flipud, d.fliplr, S).astype(np.float32))
            assert np.array_equal(plan["luts"][rec["lut"]], d.luts.reshape(-1))
            continue
        mosaics = [draw_mosaic(hyp, rng, nprs, S, len(files), b)]
        r = None
        if rng.random() < 0.5:
            mosaics.append(draw_mosaic(hyp, rng, nprs, S, len(files), rng.randint(0, len(files) - 1)))
            r = nprs.beta(32.0, 32.0)
        luts, ud, lr = draw_colour_flips(hyp, rng, nprs)
        assert len(s.plan.mosaics) == len(mosaics) and s.plan.r == r and np.array_equal(plan["luts"][rec["lut"]], luts.reshape(-1))
        boxes = []
        for l, mz in enumerate(mosaics):
            assert mz.indices == s.plan.mosaics[l].indices and mz.centre == s.plan.mosaics[l].centre
            ims = [load_image(files[i], S)[0] for i in mz.indices]
            sizes = [im.shape[:2] for im in ims]
            tiles = mosaic_tiles(sizes, mz.centre, S)
            lay = rec["layer"][l]
            assert np.array_equal(lay["m"], fixed_inverse(mz.M, ud, lr, S)) and lay["n_tiles"] == 4 and lay["fill"] == 0
            for k in range(4):
                t = lay["tile"][k]
                assert [t[f] for f in ("h", "w", "x0", "y0", "x1", "y1", "dx", "dy")] == [*sizes[k], *tiles[k]]
                assert np.array_equal(s.items[4 * l + k].pixels, ims[k])
            boxes.append(mosaic_boxes([read_labels(_label_path(files[i])) for i in mz.indices], sizes, tiles, mz.M, mz.s, S))
        want = finish_labels(np.concatenate(boxes), S, ud, lr)
        assert np.array_equal(plan["labels"][b][:, 1:], want.astype(np.float32))


def test_mosaic_zero_plans_and_draws_what_augment_alone_does(toy):
    def plans(**kw):
        src = ImageFolderSource(toy, 64, "cuda:0", seed=3, workers=0, augment={}, **kw)
        items = src._take(5)
        return [it.path for it in items], src._augment_plan(items), src._aug_rng.getstate()
    a, b = plans(), plans(mosaic=0, mixup=0.0)
    assert a[0] == b[0] and np.array_equal(a[1]["m"], b[1]["m"]) and np.array_equal(a[1]["luts"], b[1]["luts"]) and a[2] == b[2]


def test_loader_refusals(toy):
    for kw, what in [(dict(mosaic=0.5), "needs augment"), (dict(mosaic=0.5, augment={}, data_name="raw"), "raw"),
                     (dict(mixup=0.5, augment={}), "needs mosaic"), (dict(mosaic=1.5, augment={}), "probability"),
                     (dict(mosaic=-0.1, augment={}), "probability"), (dict(mosaic=1, mixup=2, augment={}), "probability"),
                     (dict(mosaic="1", augment={}), "probability"), (dict(mosaic=float("nan"), augment={}), "probability")]:
        with pytest.raises(ValueError, match=what):
            ImageFolderSource(toy, 64, "cuda:0", workers=0, **kw)
    with pytest.raises(RuntimeError, match="no CPU path"):
        ImageFolderSource(toy, 64, "cpu", workers=0, augment={}, mosaic=1.0)
    src = ImageFolderSource(toy, 64, "cuda:0", workers=0, augment={}, mosaic=1)
    assert src.mosaic == 1.0 and src.mixup == 0.0 and src.describe().endswith(", mosaic 1")


def test_hyp_still_warns_on_mosaic_and_keeps_its_keys():
    with warnings.catch_warnings(record=True) as w:
        warnings.simplefilter("always")
        h = Hyp(dict(mosaic=1.0, mixup=0.1, degrees=3))
    assert len(w) == 1 and "mosaic" in str(w[0].message) and len(h.as_dict()) == 10 and "mosaic" not in h.as_dict()


def test_train_cli_parses_mosaic_and_mixup(toy, capsys):
    from adaptiveisp_amd.train import parse_args
    a = parse_args(["--data", toy, "--augment"])
    assert a.mosaic == 0.0 and a.mixup == 0.0
    a = parse_args(["--data", toy, "--augment", "--mosaic", "1", "--mixup", "0.2"])
    assert a.mosaic == 1.0 and a.mixup == 0.2
    for bad in (["--data", toy, "--mosaic", "1"], ["--data", toy, "--augment", "--mixup", "0.2"],
                ["--data", toy, "--augment", "--mosaic", "1.5"], ["--data", toy, "--augment", "--mosaic", "1", "--mixup", "-1"]):
        with pytest.raises(SystemExit) as e:
            parse_args(bad)
        assert e.value.code == 2
    capsys.readouterr()


# ---------------------------------------------------------------------------------------------- C entry and binding
def _one(**over):
    rec = np.zeros(1, _lib.MOSAIC_DESC)
    rec["n_layers"], rec["lut"], rec["mix"] = 1, -1, 65536
    lay = rec[0]["layer"][0]
    lay["m"], lay["n_tiles"] = (65536, 0, 0, 0, 65536, 0), 1
    t = lay["tile"][0]
    t["h"], t["w"], t["x1"], t["y1"] = 4, 4, 4, 4
    for k, v in over.items():
        where = rec if k in ("n_layers", "mix", "lut") else lay if k in ("m", "fill", "n_tiles") else t
        where[k] = v
    return rec


def test_wrapper_record_checks():
    _lib._check_mosaic_records(_one(), 48, 0)
    for over, what in [(dict(n_layers=0), "n_layers"), (dict(n_layers=3), "n_layers"), (dict(mix=-1), "mix"), (dict(mix=65537), "mix"),
                       (dict(n_tiles=5), "n_tiles"), (dict(n_tiles=-1), "n_tiles"), (dict(lut=0), "table index"), (dict(lut=-2), "table index"),
                       (dict(fill=1 << 24), "fill"), (dict(m=(1 << 40, 0, 0, 0, 65536, 0)), "2\\^40"), (dict(h=-1), "size"),
                       (dict(w=32769), "size"), (dict(x1=5), "maps outside"), (dict(dy=1), "maps outside"), (dict(y1=-1), "maps outside"),
                       (dict(src_offset=-1), "outside src"), (dict(src_offset=1), "outside src")]:
        with pytest.raises(_lib.AdaispError, match=what):
            _lib._check_mosaic_records(_one(**over), 48, 0)
    # what a record does not use is not looked at: layer 1 of a one-layer record, tiles from n_tiles on
    rec = _one()
    rec[0]["layer"][1]["n_tiles"], rec[0]["layer"][0]["tile"][2]["h"] = 9, -5
    _lib._check_mosaic_records(rec, 48, 0)


def test_header_exports_and_descriptor_layout():
    hdr = open(os.path.join(ROOT, "include", "adaisp.h")).read()
    assert "int adaisp_mosaic_u8(" in hdr and all(f"}} adaisp_mosaic_{k};" in hdr for k in ("tile", "layer", "desc"))
    assert re.search(r"#define\s+ADAISP_ABI_VERSION\s+9\b", hdr)
    assert "adaisp_mosaic_u8" in _lib.EXPORTS and hasattr(_lib.load(), "adaisp_mosaic_u8") and _lib.ABI_VERSION == 9
    t, l, d = _lib.MOSAIC_TILE, _lib.MOSAIC_LAYER, _lib.MOSAIC_DESC
    assert (t.itemsize, l.itemsize, d.itemsize) == (40, 216, 448)
    assert [t.fields[n][1] for n in ("src_offset", "h", "w", "x0", "y0", "x1", "y1", "dx", "dy")] == [0, 8, 12, 16, 20, 24, 28, 32, 36]
    assert [l.fields[n][1] for n in ("m", "fill", "n_tiles", "tile")] == [0, 48, 52, 56]
    assert [d.fields[n][1] for n in ("layer", "n_layers", "mix", "lut", "reserved")] == [0, 432, 436, 440, 444]
    src = open(os.path.join(ROOT, "adaptiveisp_amd", "csrc", "isp_augment.hip")).read()
    m = re.search(r"sizeof\(adaisp_mosaic_tile\) == (\d+) && sizeof\(adaisp_mosaic_layer\) == (\d+) && sizeof\(adaisp_mosaic_desc\) == (\d+)", src)
    assert m and [int(v) for v in m.groups()] == [40, 216, 448]


def test_record_helpers_fill_what_a_hand_filled_record_holds():
    """augment.fill_mosaic_layer / fill_single_layer against records filled field by field from mosaic_tiles."""
    S, rng, rs = 64, random.Random(11), np.random.RandomState(11)
    hyp = Hyp(degrees=10, shear=5, flipud=0.5)
    mz = draw_mosaic(hyp, rng, rs, S, 9, 4)
    sizes = [(64, 40), (33, 64), (64, 64), (17, 29)]
    tiles = mosaic_tiles(sizes, mz.centre, S)
    m = fixed_inverse(mz.M, True, False, S)
    got, want = np.zeros(1, _lib.MOSAIC_DESC), np.zeros(1, _lib.MOSAIC_DESC)
    fill_mosaic_layer(got[0]["layer"][1], m, sizes, tiles)
    lay = want[0]["layer"][1]
    lay["m"], lay["n_tiles"] = m, 4
    for k in range(4):
        t = lay["tile"][k]
        t["h"], t["w"] = sizes[k]
        t["x0"], t["y0"], t["x1"], t["y1"], t["dx"], t["dy"] = tiles[k]
    assert got.tobytes() == want.tobytes() and all(np.array_equal(got[n], want[n]) for n in _lib.MOSAIC_DESC.names)
    assert got[0]["layer"][1]["tile"]["x1"].tolist() == tiles[:, 2].tolist() and (got[0]["layer"][0]["n_tiles"], got[0]["mix"]) == (0, 0)
    # a single letterboxed image: one tile over its own rectangle, moved by (left, top)
    d = draw(hyp, rng, rs, S)
    m, (h, w, top, left) = fixed_inverse(d.M, d.flipud, d.fliplr, S), (31, 44, 9, 3)
    got, want = np.zeros(1, _lib.MOSAIC_DESC), np.zeros(1, _lib.MOSAIC_DESC)
    for r in (got, want):
        r["n_layers"], r["lut"], r["mix"] = 1, -1, _lib.MOSAIC_MIX_ONE
    fill_single_layer(got[0]["layer"][0], m, h, w, top, left)
    lay = want[0]["layer"][0]
    lay["m"], lay["n_tiles"] = m, 1
    t = lay["tile"][0]
    t["h"], t["w"], t["dx"], t["dy"] = h, w, left, top
    t["x0"], t["y0"], t["x1"], t["y1"] = left, top, left + w, top + h
    assert got.tobytes() == want.tobytes() and got[0]["layer"][0]["tile"][0]["x1"] == 47 and got[0]["layer"][0]["tile"][0]["y1"] == 40
    _lib._check_mosaic_records(got, h * w * 3, 0)
    with pytest.raises(_lib.AdaispError, match="outside src"):
        _lib._check_mosaic_records(got, h * w * 3 - 1, 0)
