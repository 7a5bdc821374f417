"""adaisp_mosaic_u8 (csrc/isp_augment.hip) on the MI355X, bit for bit against the numpy int64 restatement
tests/_mosaicref.py: batches of five at S = 64 (dword stores) and S = 50 (byte stores) mixing one- and two-layer images, 0 to
4 tiles, strong maps and half-pixel translations, every kind of mix, tables on and off, odd source offsets, both fills; a
one-layer one-tile record against adaisp_augment_u8; the reference's own canvas and mixup from tests/golden/mosaic_aug.npz;
absent tiles; the error codes; then ImageFolderSource(mosaic=..., mixup=...) on a toy PNG folder and the training command line."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import _augref as A
import _mosaicref as R
from adaptiveisp_amd import _lib
from adaptiveisp_amd.augment import fill_mosaic_layer, fill_single_layer, fixed_inverse, mix_q16, mosaic_tiles
from adaptiveisp_amd.data import ImageFolderSource
from test_augment_host import _write_pngs, affine
from test_gpu_augment import _launch as augment_launch, _maps, _rand_u8, _tables
from test_mosaic_host import CASES, GREY, MIXUPS, case, crop_map, records_of

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GUARD, GUARD_BYTES = 0xA5, 64
STRONG = dict(degrees=10, shear=5, scale=0.5, translate=0.1, flipud=0.5)


def _run(src, rec, tables, S, n_layers=2, dst_shift=0, check=True):
    """One launch over the host bytes `src` into a guarded destination (`dst_shift` bytes past a 64-byte boundary)."""
    B = len(rec)
    n = B * S * S * 3
    buf = torch.full((GUARD_BYTES + dst_shift + n + GUARD_BYTES,), GUARD, dtype=torch.uint8, device=DEV)
    out = buf[GUARD_BYTES + dst_shift:GUARD_BYTES + dst_shift + n]
    luts = None if tables is None else torch.from_numpy(tables.reshape(-1).copy()).to(DEV)
    got = _lib.mosaic_u8(torch.from_numpy(src.copy()).to(DEV), torch.from_numpy(rec.view(np.uint8).copy()).to(DEV), luts, S,
                         n_layers=n_layers, out=out, records=rec if check else None)
    assert got.data_ptr() == out.data_ptr()
    host = buf.cpu().numpy()
    assert (host[:GUARD_BYTES + dst_shift] == GUARD).all() and (host[GUARD_BYTES + dst_shift + n:] == GUARD).all()
    return host[GUARD_BYTES + dst_shift:GUARD_BYTES + dst_shift + n].reshape(B, S, S, 3)


class Packer:
    """Source images packed with `gap` filler bytes before each (odd: odd offsets)."""

    def __init__(self, gap=3):
        self.gap, self.chunks, self.size = gap, [], 0

    def add(self, im):
        self.chunks += [np.full(self.gap, 77, np.uint8), im.reshape(-1)]
        self.size += self.gap + im.size
        return self.size - im.size

    def bytes(self):
        return np.concatenate(self.chunks)


def _layer(lay, pack, imgs, centre, S, m, fill, n_tiles):
    """The first n_tiles of the four-image mosaic of `imgs` around `centre` into the layer record."""
    sizes = [im.shape[:2] for im in imgs]
    fill_mosaic_layer(lay, m, sizes[:n_tiles], mosaic_tiles(sizes, centre, S)[:n_tiles])
    lay["fill"] = fill
    for k in range(n_tiles):
        lay["tile"][k]["src_offset"] = pack.add(imgs[k])


def _half(S, ox=0, oy=0):
    """Scale 1, the crop's translation plus half a pixel each way: every output pixel has taps in four canvas pixels, so the
    pixels along both seams through the centre blend two tiles (or a tile and the fill)."""
    return (65536, 0, (S // 2 + ox) * 65536 + 32768, 0, 65536, (S // 2 + oy) * 65536 + 32768)


def _batch_of_five(S, fill, seed):
    rs = np.random.RandomState(seed)
    q, t = S // 2, 3 * S // 4
    sizes = [(S, 5 * S // 8), (t, S), (S, S), (S, q + 1), (q - 1, S), (q - 3, q // 2), (S // 4, q - 1), (7, 5)]
    imgs = [_rand_u8(rs, h, w) for h, w in sizes]
    strong = fixed_inverse(affine(2 * S, 10.0, 0.5, 5.0, 0.25, 0.25), True, True, S)       # C = -S, T = S / 2: the canvas's
    zoom = fixed_inverse(affine(2 * S, -7.0, 1.4, 3.0, 0.27, 0.22), False, True, S)
    pack, rec = Packer(), np.zeros(5, _lib.MOSAIC_DESC)
    # image: (layers: (images, centre, map, tiles)), mix, table
    plan = [([([0, 1, 2, 3], (S - 5, S + 3), strong, 4)], 65536, 0),
            ([([4, 5, 6, 7], (S, S), _half(S), 4), ([3, 2, 1, 0], (q + 1, S + q - 2), strong, 3)], 30000, -1),
            ([([5, 1, 6, 3], (S + 7, S - 9), zoom, 2), ([2, 0, 4, 7], (S, q), _half(S, 3, -2), 1)], 1, 1),
            ([([0, 1, 2, 3], (S, S), strong, 0), ([6, 7, 5, 4], (S - 1, S + 1), _half(S, -4, 5), 4)], 0, -1),
            ([([7, 6, 5, 4], (S + 2, S + 2), _half(S), 1), ([1, 3, 0, 2], (S, S), zoom, 2)], 65536, 0)]
    for b, (layers, mix, lut) in enumerate(plan):
        rec[b]["n_layers"], rec[b]["mix"], rec[b]["lut"] = len(layers), mix, lut
        for l, (idx, centre, m, n) in enumerate(layers):
            _layer(rec[b]["layer"][l], pack, [imgs[i] for i in idx], centre, S, m, fill, n)
    pack.add(np.zeros(0, np.uint8))
    return pack.bytes(), rec


@pytest.mark.parametrize("fill", [0, 0x727272])
@pytest.mark.parametrize("S", [64, 50])
def test_kernel_matches_the_restatement_bit_for_bit(S, fill):
    src, rec = _batch_of_five(S, fill, S + fill % 7)
    tables = _tables(S)
    assert sorted({int(n) for r in rec for n in r["layer"]["n_tiles"][:r["n_layers"]]}) == [0, 1, 2, 3, 4]
    assert set(rec["n_layers"].tolist()) == {1, 2} and set(rec["mix"].tolist()) == {0, 1, 30000, 65536}
    offsets = [int(o) for r in rec for lay in r["layer"][:r["n_layers"]] for o in lay["tile"]["src_offset"][:lay["n_tiles"]]]
    assert sum(o % 2 for o in offsets) > 4 and {o % 4 for o in offsets} == {0, 1, 2, 3}              # odd ones, every alignment
    got = _run(src, rec, tables, S)
    want = R.batch(src, rec, S, tables)
    assert np.array_equal(got, want), [b for b in range(5) if not np.array_equal(got[b], want[b])]
    assert len({got[b].tobytes() for b in range(5)}) == 5
    # a launch of one layer makes every image from its layer 0 alone
    one = rec.copy()
    one["n_layers"] = 1
    got1 = _run(src, one, tables, S, n_layers=1)
    assert np.array_equal(got1, R.batch(src, one, S, tables)) and np.array_equal(got1, R.batch(src, rec, S, tables, n_layers=1))
    assert np.array_equal(got1[0], got[0]) and not np.array_equal(got1[1], got[1])
    pad = np.array(A.fill_triple(fill), np.uint8)
    assert (got1[3] == pad).all()                                      # no tile: the fill alone


def test_half_pixel_seams_blend_two_tiles():
    """Along the seam column the kernel's pixel is the mean of the reference canvas's pixels on both sides."""
    g = case("large_64")
    S = 64
    rec, src = records_of(g, _half(S), gap=1)
    got = _run(src, rec, None, S)[0]
    c = g["canvas"].astype(np.int64)
    y, x = np.mgrid[S // 2:3 * S // 2, S // 2:3 * S // 2]
    want = ((256 * (c[y, x] + c[y, x + 1] + c[y + 1, x] + c[y + 1, x + 1]) + 512) >> 10).astype(np.uint8)
    xc, yc = (int(v) for v in g["centre"])
    assert S // 2 < xc < 3 * S // 2 and S // 2 < yc < 3 * S // 2        # both seams cross the frame
    assert np.array_equal(got, want)


@pytest.mark.parametrize("S", [64, 50])
def test_one_layer_one_tile_is_adaisp_augment_u8_byte_for_byte(S):
    rs = np.random.RandomState(S)
    sizes = [(1, 1), (1, 40), (40, 1), (37, min(64, S)), (min(64, S), min(64, S)), (20, 30)]
    imgs = [_rand_u8(rs, h, w) for h, w in sizes]
    place = [((S - h) // 2, (S - w) // 2) for h, w in sizes[:5]] + [(7, 9)]
    maps, tables, fill = _maps(S), _tables(S), 0x302010
    for shift in (0, 3, 4):
        m = [maps[(k + shift) % 6] for k in range(6)]
        lut = [(k + shift) % 3 - 1 for k in range(6)]
        want, arec = augment_launch(imgs, place, m, lut, tables, S, fill)
        pack, rec = Packer(), np.zeros(6, _lib.MOSAIC_DESC)
        rec["n_layers"], rec["lut"], rec["mix"] = 1, lut, 65536
        for b, (im, (top, left)) in enumerate(zip(imgs, place)):
            lay = rec[b]["layer"][0]
            fill_single_layer(lay, m[b], im.shape[0], im.shape[1], top, left)
            lay["fill"], lay["tile"][0]["src_offset"] = fill, pack.add(im)
        pack.add(np.zeros(0, np.uint8))
        for n_layers in (1, 2):
            assert np.array_equal(_run(pack.bytes(), rec, tables, S, n_layers=n_layers), want), (shift, n_layers)


@pytest.mark.parametrize("S", [32, 64])
def test_crop_map_gives_the_reference_canvas(S):
    names = [n for n in CASES if n.endswith(f"_{S}")]
    pack, rec, want = Packer(gap=1), np.zeros(len(names), _lib.MOSAIC_DESC), []
    for b, name in enumerate(names):
        g = case(name)
        one, src = records_of(g, crop_map(S))
        one["layer"]["tile"]["src_offset"] += pack.add(src)
        rec[b] = one[0]
        want.append(g["canvas"][S // 2:3 * S // 2, S // 2:3 * S // 2])
    pack.add(np.zeros(0, np.uint8))
    assert len(names) == 6 and (rec["layer"]["fill"][:, 0] == GREY).all()
    assert np.array_equal(_run(pack.bytes(), rec, None, S, n_layers=1), np.stack(want))


def test_mix_tracks_the_reference_mixup_within_one_step():
    """mix = rint(65536 r): the weight is off by at most 2^-17, the value by 255 * 2^-17 << 1 before the floor, so floor
    against the reference's floor differs by at most one step."""
    for S in (32, 64):
        names = [n for n in MIXUPS if n.startswith(f"mixup_{S}_")]
        pack, rec, want = Packer(), np.zeros(len(names), _lib.MOSAIC_DESC), []
        for b, name in enumerate(names):
            g = case(name)
            rs = np.random.RandomState(int(g["seed"]))
            rec[b]["n_layers"], rec[b]["lut"], rec[b]["mix"] = 2, -1, mix_q16(float(g["r"]))
            for l in range(2):
                im = rs.randint(0, 256, size=(S, S, 3)).astype(np.uint8)
                lay = rec[b]["layer"][l]
                fill_single_layer(lay, A.IDENTITY, S, S, 0, 0)
                lay["tile"][0]["src_offset"] = pack.add(im)
            want.append(g["mixed"])
        pack.add(np.zeros(0, np.uint8))
        got = _run(pack.bytes(), rec, None, S)
        delta = np.abs(got.astype(np.int64) - np.stack(want).astype(np.int64))
        print(f"S = {S}: max |kernel - reference mixup| = {delta.max()}, differing {np.count_nonzero(delta)} of {delta.size}")
        assert np.array_equal(got, R.batch(pack.bytes(), rec, S)) and delta.max() <= 1


def test_tile_outside_its_source_or_past_src_reads_as_fill():
    """The source buffer is sized exactly: its last tile ends on its last byte. Absent tiles are never read from."""
    rs, S, fill = np.random.RandomState(9), 64, 0x302010
    a, b = _rand_u8(rs, 20, 30), _rand_u8(rs, 16, 16)
    src = np.concatenate([a.reshape(-1), b.reshape(-1)])
    rec = np.zeros(4, _lib.MOSAIC_DESC)
    rec["n_layers"], rec["lut"], rec["mix"] = 1, -1, 65536
    for r in rec:
        lay = r["layer"][0]
        lay["m"], lay["fill"], lay["n_tiles"] = A.IDENTITY, fill, 2
        t = lay["tile"][0]
        t["h"], t["w"], t["x0"], t["y0"], t["x1"], t["y1"], t["dx"], t["dy"] = 20, 30, 2, 3, 32, 23, 2, 3
        t = lay["tile"][1]
        t["src_offset"], t["h"], t["w"] = a.size, 16, 16
        t["x0"], t["y0"], t["x1"], t["y1"], t["dx"], t["dy"] = 40, 40, 56, 56, 40, 40
    rec[1]["layer"][0]["tile"][0]["x1"] = 33                           # one column more than the source has
    rec[2]["layer"][0]["tile"][1]["src_offset"] = a.size + 1           # its last byte is one past src
    rec[3]["layer"][0]["tile"][0]["dy"] = 4                            # row -1 of the source
    rec[3]["layer"][0]["tile"][1]["src_offset"] = 1 << 40
    got = _run(src, rec, None, S, check=False)
    pad = np.array(A.fill_triple(fill), np.uint8)
    whole = np.empty((S, S, 3), np.uint8)
    whole[...] = pad
    whole[3:23, 2:32], whole[40:56, 40:56] = a, b
    no_a, no_b = whole.copy(), whole.copy()
    no_a[3:23, 2:32], no_b[40:56, 40:56] = pad, pad
    assert np.array_equal(got[0], whole) and np.array_equal(got[1], no_a) and np.array_equal(got[2], no_b)
    assert (got[3] == pad).all() and np.array_equal(got, R.batch(src, rec, S))
    for k, what in ((1, "maps outside"), (2, "outside src"), (3, "maps outside")):
        with pytest.raises(_lib.AdaispError, match=what):
            _lib.mosaic_u8(torch.from_numpy(src).to(DEV), torch.from_numpy(rec[k:k + 1].view(np.uint8).copy()).to(DEV), None, S,
                           records=rec[k:k + 1])


def test_error_codes_without_launching():
    L = _lib.load()
    src = torch.zeros(256, dtype=torch.uint8, device=DEV)
    desc = torch.zeros(_lib.MOSAIC_DESC.itemsize, dtype=torch.uint8, device=DEV)
    out = torch.full((8 * 8 * 3,), GUARD, dtype=torch.uint8, device=DEV)

    def call(s=src.data_ptr(), d=desc.data_ptr(), luts=None, n_luts=0, o=out.data_ptr(), B=1, S=8, n_layers=1):
        return L.adaisp_mosaic_u8(s, src.numel(), d, luts, n_luts, o, B, S, n_layers, None)

    assert call(s=None) == -1 and call(d=None) == -1 and call(o=None) == -1 and call(B=0) == -1 and call(S=0) == -1
    assert call(n_luts=1) == -1 and call(luts=src.data_ptr(), n_luts=-1) == -1
    assert call(n_layers=0) == -1 and call(n_layers=3) == -1
    assert call(B=65536) == -4 and call(S=32769) == -4
    torch.cuda.synchronize()
    assert (out.cpu().numpy() == GUARD).all()                    # nothing was launched
    rec = np.zeros(1, _lib.MOSAIC_DESC)
    rec["n_layers"], rec["lut"] = 1, -1
    for over, what in [(dict(n_layers=3), "n_layers"), (dict(mix=65537), "mix"), (dict(mix=-1), "mix"), (dict(lut=0), "table index")]:
        bad = rec.copy()
        for k, v in over.items():
            bad[k] = v
        with pytest.raises(_lib.AdaispError, match=what):
            _lib.mosaic_u8(src, desc, None, 8, out=out, records=bad)
    bad = rec.copy()
    bad[0]["layer"][0]["n_tiles"] = 5
    two = rec.copy()
    two["n_layers"] = 2
    for kw, what in [(dict(records=bad), "n_tiles"), (dict(records=two, n_layers=1), "two layers"), (dict(n_layers=3), "n_layers"),
                     (dict(luts=src[:100]), "768"), (dict(out=out[:100]), "frames"), (dict(records=np.zeros(2, _lib.MOSAIC_DESC)), "records"),
                     (dict(luts=torch.zeros(768, dtype=torch.uint8)), "luts")]:
        kw = dict(dict(luts=None, out=out), **kw)
        with pytest.raises(_lib.AdaispError, match=what):
            _lib.mosaic_u8(src, desc, kw.pop("luts"), 8, **kw)
    with pytest.raises(_lib.AdaispError, match="whole number"):
        _lib.mosaic_u8(src, desc[:50], None, 8)
    torch.cuda.synchronize()
    assert (out.cpu().numpy() == GUARD).all()


def test_unaligned_destination_takes_the_byte_path():
    src, rec = _batch_of_five(64, 0x727272, 5)
    tables = _tables(5)
    want = R.batch(src, rec, 64, tables)
    for shift in (1, 2, 3):
        assert np.array_equal(_run(src, rec, tables, 64, dst_shift=shift), want), shift


# ------------------------------------------------------------------------------------------------------- the loader
SIZES = [(48, 64), (64, 40), (20, 30), (64, 64), (100, 80), (33, 17), (150, 200)]      # portrait, landscape, smaller and larger than S


@pytest.fixture(scope="module")
def toy(tmp_path_factory):
    return _write_pngs(str(tmp_path_factory.mktemp("mosaicdata")), SIZES, seed=2)


def _batches(root, counts=(3, 4, 2), **kw):
    src = ImageFolderSource(root, 64, DEV, seed=3, **kw)
    try:
        out = []
        for n in counts:
            imgs, labels, paths, shapes = src.get_next_batch(n)
            out.append((torch.stack(list(imgs)).cpu().numpy(), [lb.copy() for lb in labels], list(paths), list(shapes)))
        torch.cuda.synchronize()
        return out, src.rs.get_state()[1].copy(), src.serial, src.describe()
    finally:
        src.close()


def _same(a, b):
    return all(np.array_equal(x[0], y[0]) and len(x[1]) == len(y[1]) and all(np.array_equal(p, q) for p, q in zip(x[1], y[1]))
               and x[2] == y[2] and x[3] == y[3] for x, y in zip(a, b)) and len(a) == len(b)


@pytest.fixture(scope="module")
def mixed(toy):
    """The batches every loader test compares against: mosaic = 1, mixup = 0.5, host resize, no workers."""
    return _batches(toy, workers=0, augment=STRONG, mosaic=1, mixup=0.5)


def test_loader_equals_the_restatement_of_the_planned_records(toy, mixed):
    got, _, _, text = mixed
    assert text.startswith("lod: 7 files, augment (") and text.endswith("), mosaic 1, mixup 0.5")
    twin = ImageFolderSource(toy, 64, DEV, seed=3, workers=0, augment=STRONG, mosaic=1, mixup=0.5)   # plans only
    files, layers = sorted(twin.files), set()
    for imgs, labels, paths, shapes in got:
        samples = twin._take_samples(len(paths))
        plan = twin._mosaic_plan(samples)
        rec, at, off = plan["records"].copy(), [], 0
        for it in plan["items"]:
            at.append(off)
            off += it.pixels.size
        for b, l, t, k in plan["slots"]:
            rec[b]["layer"][l]["tile"][t]["src_offset"] = at[k]
        src = np.concatenate([it.pixels.reshape(-1) for it in plan["items"]])
        u8 = R.batch(src, rec, 64, plan["luts"])
        want = np.ascontiguousarray(u8[..., ::-1].transpose(0, 3, 1, 2)).astype(np.float32) / np.float32(255)
        assert np.array_equal(imgs, want)
        assert paths == [files[s.plan.index] for s in samples] and shapes == [None] * len(paths)
        assert all(np.array_equal(x, y) for x, y in zip(labels, plan["labels"])) and len(labels) == len(paths)
        assert (rec["layer"]["fill"] == 0).all() and all(len(s.items) == 4 * len(s.plan.mosaics) for s in samples)
        layers |= set(rec["n_layers"].tolist())
    twin.close()
    assert layers == {1, 2}


def test_loader_is_the_same_for_every_worker_count_and_resize(toy, mixed):
    for kw in (dict(workers=3), dict(workers=0, resize="device"), dict(workers=3, resize="device")):
        other, rs, serial, _ = _batches(toy, augment=STRONG, mosaic=1, mixup=0.5, **kw)
        assert _same(mixed[0], other) and np.array_equal(rs, mixed[1]) and serial == mixed[2], kw
    part, _, _, _ = _batches(toy, workers=0, augment=STRONG, mosaic=0.5, mixup=0.5)         # single images in the same launch
    part3, _, _, _ = _batches(toy, workers=3, augment=STRONG, mosaic=0.5, mixup=0.5, resize="device")
    assert _same(part, part3) and {s is None for b in part for s in b[3]} == {True, False}


def test_loader_with_mosaic_zero_is_the_augmented_loader_of_today(toy, mixed):
    for kw in (dict(), dict(data_name="coco", add_noise=True, sensor="bayer", resize="device")):
        a, rs_a, serial_a, text_a = _batches(toy, workers=0, augment=STRONG, mosaic=0, mixup=0, **kw)
        b, rs_b, serial_b, text_b = _batches(toy, workers=0, augment=STRONG, **kw)
        assert _same(a, b) and np.array_equal(rs_a, rs_b) and serial_a == serial_b and text_a == text_b and "mosaic" not in text_a
    assert not np.array_equal(mixed[0][0][0], b[0][0]) and np.array_equal(mixed[1], _batches(toy, workers=0)[1])


@pytest.mark.parametrize("kw", [dict(data_name="coco", add_noise=True), dict(data_name="coco", add_noise=True, sensor="bayer", resize="device")],
                         ids=["coco-noise", "coco-noise-bayer-device"])
def test_loader_through_the_sensor_models(toy, kw):
    a, rs_a, serial_a, _ = _batches(toy, workers=2, augment=STRONG, mosaic=1, mixup=0.5, **kw)
    plain, rs_p, serial_p, _ = _batches(toy, workers=0, **kw)
    assert np.array_equal(rs_a, rs_p) and serial_a == serial_p           # the metadata draws and noise keys of the seed
    for (imgs, labels, paths, shapes), (pimgs, _, ppaths, _) in zip(a, plain):
        assert imgs.shape == pimgs.shape == (len(paths), 3, 64, 64) and imgs.dtype == np.float32
        assert np.isfinite(imgs).all() and imgs.min() >= 0.0 and imgs.max() <= 1.0 and imgs.std() > 0
        assert paths == ppaths and shapes == [None] * len(paths)
        assert all(lb.dtype == np.float32 and lb.shape[1] == 6 for lb in labels)


def test_cli_trains_with_mosaic_and_mixup(toy):
    cache = os.path.join(ROOT, "adaptiveisp_amd", "yolo", "tuning", "mi355x.json")
    saved = open(cache, "rb").read()              # the CLI autotunes into the committed table: give it back as it was
    try:
        r = subprocess.run(["timeout", "-k", "10", "600", sys.executable, "-m", "adaptiveisp_amd.train", "--data", toy, "--augment",
                            "--mosaic", "1", "--mixup", "0.2", "--iters", "2", "--batch", "2", "--size", "64"], cwd=ROOT,
                           capture_output=True, text=True)
    finally:
        with open(cache, "wb") as f:
            f.write(saved)
    assert r.returncode == 0, r.stderr[-3000:]
    line = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1])
    assert line["data"].startswith("lod: 7 files, augment (hsv_h=0.015 ") and line["data"].endswith(", mosaic 1, mixup 0.2"), line["data"]
    last = line["last"]
    assert np.isfinite([last["agent_loss"], last["value_loss"], last["reward"]]).all(), last
