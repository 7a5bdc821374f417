"""adaisp_augment_u8 (csrc/isp_augment.hip) on the MI355X, bit for bit against the numpy int64 restatement
tests/_augref.py: small batches at S = 64 (dword stores) and S = 50 (byte stores) with sources at odd byte offsets, every
kind of map, both fills, with and without tables, guard bytes around the destination; the workload shape once; the error
codes; then ImageFolderSource(augment=...) on toy PNG datasets in every mode, and the training command line."""
import json
import os
import random
import subprocess
import sys

import numpy as np
import pytest
import torch

import _augref as R
from adaptiveisp_amd import _lib
from adaptiveisp_amd.augment import Hyp, draw, fixed_inverse, warp_labels
from adaptiveisp_amd.data import ImageFolderSource
from adaptiveisp_amd.val.loader import load_letterboxed
from test_augment_host import _write_pngs, affine

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GUARD, GUARD_BYTES = 0xA5, 64
STRONG = dict(degrees=10, shear=5, scale=0.5, translate=0.1, flipud=0.5)


def _rand_u8(rs, h, w):
    im = rs.randint(0, 256, size=(h, w, 3)).astype(np.uint8)
    im.reshape(-1)[0], im.reshape(-1)[-1] = 0, 255
    return im


def _maps(S):
    """identity, each flip, the 10 degree / 0.8 x / 5 degree shear map, a 1.5 x zoom, a translation that empties the frame."""
    far = np.eye(3)
    far[0, 2] = 3 * S
    return [fixed_inverse(np.eye(3), False, False, S), fixed_inverse(np.eye(3), False, True, S),
            fixed_inverse(np.eye(3), True, False, S), fixed_inverse(affine(S, 10.0, 0.8, 5.0), False, False, S),
            fixed_inverse(affine(S, 0.0, 1.5, 0.0, 0.47, 0.55), True, True, S), fixed_inverse(far, False, False, S)]


def _tables(seed):
    """Two tables: one as augment_hsv builds them, one of arbitrary bytes (hue entries of 180 and more included)."""
    d = draw(Hyp(hsv_h=0.5, hsv_s=0.7, hsv_v=0.4), random.Random(seed), np.random.RandomState(seed), 64)
    return np.stack([d.luts.reshape(-1), np.random.RandomState(seed).randint(0, 256, 768).astype(np.uint8)])


def _launch(imgs, place, maps, lut, tables, S, fill, gap=3, dst_shift=0, check=True):
    """Packs `imgs` with `gap` filler bytes before each (odd: odd offsets), runs one launch into a guarded destination
    (`dst_shift` bytes past a 64-byte boundary) and returns (uint8 [B,S,S,3], records)."""
    B = len(imgs)
    rec = np.zeros(B, _lib.AUGMENT_DESC)
    chunks, off = [], gap
    for b, im in enumerate(imgs):
        chunks += [np.full(gap, 77, np.uint8), im.reshape(-1)]
        rec[b]["src_offset"], rec[b]["h"], rec[b]["w"] = off, im.shape[0], im.shape[1]
        rec[b]["top"], rec[b]["left"] = place[b]
        rec[b]["m"], rec[b]["lut"] = maps[b], lut[b]
        off += gap + im.size
    src = torch.from_numpy(np.concatenate(chunks + [np.full(gap, 77, np.uint8)])).to(DEV)
    desc = torch.from_numpy(rec.view(np.uint8).copy()).to(DEV)
    luts = None if tables is None else torch.from_numpy(tables.reshape(-1).copy()).to(DEV)
    n = B * S * S * 3
    buf = torch.full((GUARD_BYTES + dst_shift + n + GUARD_BYTES,), GUARD, dtype=torch.uint8, device=DEV)
    out = buf[GUARD_BYTES + dst_shift:GUARD_BYTES + dst_shift + n]
    got = _lib.augment_u8(src, desc, luts, S, fill=fill, out=out, records=rec if check else None)
    assert got.data_ptr() == out.data_ptr()
    host = buf.cpu().numpy()
    assert (host[:GUARD_BYTES + dst_shift] == GUARD).all() and (host[GUARD_BYTES + dst_shift + n:] == GUARD).all()
    return host[GUARD_BYTES + dst_shift:GUARD_BYTES + dst_shift + n].reshape(B, S, S, 3), rec


def _expect(imgs, rec, tables, S, fill):
    return np.stack([R.augment(im, int(r["top"]), int(r["left"]), r["m"].tolist(), S, fill,
                               None if r["lut"] < 0 else tables[r["lut"]]) for im, r in zip(imgs, rec)])


@pytest.mark.parametrize("fill", [0, 0x727272])
@pytest.mark.parametrize("S", [64, 50])
def test_kernel_matches_the_restatement_bit_for_bit(S, fill):
    """Sources 1 x 1, 1 x 40, 40 x 1, 37 x 64, 64 x 64 and one placed off-centre (the two 64-pixel sides are S at S = 50,
    so that they still fit); six launches pair every image with every map, and with no table and each of two tables."""
    rs = np.random.RandomState(S + fill % 7)
    sizes = [(1, 1), (1, 40), (40, 1), (37, min(64, S)), (min(64, S), min(64, S)), (20, 30)]
    imgs = [_rand_u8(rs, h, w) for h, w in sizes]
    place = [((S - h) // 2, (S - w) // 2) for h, w in sizes[:5]] + [(7, 9)]
    maps, tables = _maps(S), _tables(S)
    for shift in range(6):
        m = [maps[(k + shift) % 6] for k in range(6)]
        lut = [(k + shift) % 3 - 1 for k in range(6)]
        got, rec = _launch(imgs, place, m, lut, tables, S, fill)
        want = _expect(imgs, rec, tables, S, fill)
        assert np.array_equal(got, want), (shift, [b for b in range(6) if not np.array_equal(got[b], want[b])])
    frames = np.stack([R.letterboxed(im, S, t, l, fill) for im, (t, l) in zip(imgs, place)])
    got, _ = _launch(imgs, place, [maps[0]] * 6, [-1] * 6, None, S, fill)
    assert np.array_equal(got, frames)                          # identity, no table: the letterboxed frames themselves
    got, _ = _launch(imgs, place, [maps[5]] * 6, [-1] * 6, None, S, fill)
    assert (got == np.array(R.fill_triple(fill), np.uint8)).all()


def test_unaligned_destination_takes_the_byte_path():
    rs = np.random.RandomState(5)
    imgs, place, S = [_rand_u8(rs, 37, 64), _rand_u8(rs, 20, 30)], [(13, 0), (7, 9)], 64
    maps, tables = _maps(S), _tables(5)
    for shift in (1, 2, 3):
        got, rec = _launch(imgs, place, [maps[3], maps[4]], [1, 0], tables, S, 0x727272, gap=1, dst_shift=shift)
        assert np.array_equal(got, _expect(imgs, rec, tables, S, 0x727272))


def test_descriptor_that_does_not_fit_is_all_fill_and_never_read():
    rs = np.random.RandomState(6)
    S, fill = 64, 0x302010
    imgs = [_rand_u8(rs, 30, 40), _rand_u8(rs, 30, 40), _rand_u8(rs, 30, 40), _rand_u8(rs, 8, 8)]
    ident = _maps(S)[0]
    got, rec = _launch(imgs, [(35, 0), (0, 25), (-1, 0), (3, 3)], [ident] * 4, [0, -1, 0, -1], _tables(6), S, fill, check=False)
    pad = np.array(R.fill_triple(fill), np.uint8)
    want = R.colour(np.broadcast_to(pad, (S, S, 3)), _tables(6)[0])
    assert np.array_equal(got[0], want) and (got[1] == pad).all() and np.array_equal(got[2], want)
    assert np.array_equal(got[3], R.letterboxed(imgs[3], S, 3, 3, fill))
    # a source that does not lie inside src, and a table index past the tables: fill, and no colour change
    B = 2
    rec = np.zeros(B, _lib.AUGMENT_DESC)
    rec["h"], rec["w"], rec["m"] = 8, 8, ident
    rec["src_offset"], rec["lut"] = [1 << 40, 0], [-1, 7]
    src = torch.from_numpy(imgs[3].reshape(-1).copy()).to(DEV)
    out = _lib.augment_u8(src, torch.from_numpy(rec.view(np.uint8).copy()).to(DEV), torch.from_numpy(_tables(6).reshape(-1)).to(DEV),
                          S, fill=fill).cpu().numpy()
    assert (out[0] == pad).all() and np.array_equal(out[1], R.letterboxed(imgs[3], S, 0, 0, fill))
    with pytest.raises(_lib.AdaispError, match="outside src"):
        _lib.augment_u8(src, torch.from_numpy(rec.view(np.uint8).copy()).to(DEV), None, S, records=rec)


def test_workload_shape():
    """B = 8 at S = 512: drawn maps and tables, sources of several sizes."""
    S, B = 512, 8
    rs, rng = np.random.RandomState(8), random.Random(8)
    hyp = Hyp(STRONG)
    sizes = [(512, 512), (384, 512), (512, 341), (300, 400), (512, 512), (1, 512), (200, 150), (512, 384)]
    imgs = [_rand_u8(rs, h, w) for h, w in sizes]
    place = [((S - h) // 2, (S - w) // 2) for h, w in sizes]
    draws = [draw(hyp, rng, rs, S) for _ in range(B)]
    maps = [fixed_inverse(d.M, d.flipud, d.fliplr, S) for d in draws]
    tables = np.stack([d.luts.reshape(-1) for d in draws])
    got, rec = _launch(imgs, place, maps, list(range(B)), tables, S, 0, gap=5)
    want = _expect(imgs, rec, tables, S, 0)
    assert np.array_equal(got, want), [b for b in range(B) if not np.array_equal(got[b], want[b])]
    assert len({got[b].tobytes() for b in range(B)}) == B and all(got[b].any() for b in range(B))


def test_error_codes_without_launching():
    L = _lib.load()
    src = torch.zeros(256, dtype=torch.uint8, device=DEV)
    desc = torch.zeros(_lib.AUGMENT_DESC.itemsize, dtype=torch.uint8, device=DEV)
    out = torch.full((8 * 8 * 3,), GUARD, dtype=torch.uint8, device=DEV)

    def call(s=src.data_ptr(), d=desc.data_ptr(), luts=None, n_luts=0, o=out.data_ptr(), B=1, S=8, fill=0):
        return L.adaisp_augment_u8(s, src.numel(), d, luts, n_luts, o, B, S, fill, None)

    assert call(s=None) == -1 and call(d=None) == -1 and call(o=None) == -1 and call(B=0) == -1 and call(S=0) == -1
    assert call(n_luts=1) == -1 and call(luts=src.data_ptr(), n_luts=-1) == -1 and call(fill=1 << 24) == -1
    assert call(B=65536) == -4 and call(S=32769) == -4
    torch.cuda.synchronize()
    assert (out.cpu().numpy() == GUARD).all()                    # nothing was launched
    for bad, what in [(dict(luts=src[:100]), "768"), (dict(out=out[:100]), "frames"), (dict(fill=-1), "fill"),
                      (dict(records=np.zeros(2, _lib.AUGMENT_DESC)), "records"), (dict(luts=torch.zeros(768, dtype=torch.uint8)), "luts")]:
        kw = dict(dict(luts=None, out=out), **bad)
        with pytest.raises(_lib.AdaispError, match=what):
            _lib.augment_u8(src, desc, kw.pop("luts"), 8, **kw)
    with pytest.raises(_lib.AdaispError, match="whole number"):
        _lib.augment_u8(src, desc[:50], None, 8)


# ------------------------------------------------------------------------------------------------------- the loader
SIZES = [(48, 64), (64, 40), (20, 30), (64, 64), (100, 80), (33, 17), (150, 200)]      # one portrait, one smaller than S


@pytest.fixture(scope="module")
def toy(tmp_path_factory):
    return _write_pngs(str(tmp_path_factory.mktemp("augdata")), SIZES, seed=2)


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


def test_loader_lod_equals_the_restatement_of_the_planned_maps(toy):
    got, _, _, text = _batches(toy, workers=0, augment=STRONG)
    assert text.startswith("lod: 7 files, augment (") and "degrees=10" in text
    twin = ImageFolderSource(toy, 64, DEV, seed=3, workers=0, augment=STRONG)       # plans only: it never makes a batch
    plain, _, _, _ = _batches(toy, workers=0)
    changed = 0
    for (imgs, labels, paths, shapes), (_, plain_labels, plain_paths, plain_shapes) in zip(got, plain):
        plan = twin._augment_plan(twin._take(len(paths)))
        assert paths == plain_paths and shapes == plain_shapes
        for b, p in enumerate(paths):
            im, (top, left), _, lb, _ = load_letterboxed(p, 64)
            d = plan["draws"][b]
            u8 = R.augment(im, top, left, fixed_inverse(d.M, d.flipud, d.fliplr, 64).tolist(), 64, 0, d.luts.reshape(-1))
            want = np.ascontiguousarray(u8[..., ::-1].transpose(2, 0, 1)).astype(np.float32) / np.float32(255)
            assert np.array_equal(imgs[b], want), p
            wl = warp_labels(lb, d.M, d.s, d.flipud, d.fliplr, 64)
            assert labels[b].shape == (len(wl), 6) and np.array_equal(labels[b][:, 1:], wl.astype(np.float32))
            changed += len(labels[b]) != len(plain_labels[b]) or not np.array_equal(labels[b], plain_labels[b])
    twin.close()
    assert changed > 0


def test_loader_device_resize_and_workers_give_the_same_batches(toy):
    host, _, _, _ = _batches(toy, workers=0, augment=STRONG)
    dev, _, _, text = _batches(toy, workers=0, augment=STRONG, resize="device")
    four, _, _, _ = _batches(toy, workers=4, augment=STRONG)
    assert "device resize" in text and _same(host, dev) and _same(host, four)
    assert not np.array_equal(host[0][0], _batches(toy, workers=0)[0][0][0])


def test_loader_without_augment_is_what_it_was(toy):
    for kw in (dict(), dict(data_name="coco", add_noise=True), dict(sensor="bayer", resize="device")):
        a, rs_a, serial_a, text_a = _batches(toy, workers=0, augment=None, **kw)
        b, rs_b, serial_b, text_b = _batches(toy, workers=0, **kw)
        assert _same(a, b) and np.array_equal(rs_a, rs_b) and serial_a == serial_b and text_a == text_b and "augment" not in text_a


@pytest.mark.parametrize("kw", [dict(data_name="coco", add_noise=True), dict(data_name="coco", add_noise=True, sensor="bayer"),
                                dict(sensor="bayer"), dict(data_name="coco", add_noise=True, sensor="bayer", resize="device")],
                         ids=["coco-noise", "coco-noise-bayer", "lod-bayer", "coco-noise-bayer-device"])
def test_loader_through_the_sensor_models(toy, kw):
    a, rs_a, serial_a, _ = _batches(toy, workers=0, augment=STRONG, **kw)
    b, rs_b, serial_b, _ = _batches(toy, workers=2, augment=STRONG, **kw)
    plain, rs_p, serial_p, _ = _batches(toy, workers=0, **kw)
    assert _same(a, b)                                             # one seed, one sequence
    assert np.array_equal(rs_a, rs_p) and np.array_equal(rs_b, rs_p) and serial_a == serial_p == serial_b    # metadata draws, noise keys
    for (imgs, labels, paths, shapes), (pimgs, _, ppaths, pshapes) in zip(a, plain):
        assert imgs.shape == pimgs.shape == (len(paths), 3, 64, 64) and imgs.dtype == np.float32
        assert np.isfinite(imgs).all() and imgs.min() >= 0.0 and imgs.max() <= 1.0
        assert paths == ppaths and shapes == pshapes and not np.array_equal(imgs, pimgs)
        assert all(lb.dtype == np.float32 and lb.shape[1] == 6 for lb in labels)


def test_cli_trains_with_augmentation(toy):
    cache = os.path.join(ROOT, "adaptiveisp_amd", "yolo", "tuning", "mi355x.json")
    saved = open(cache, "rb").read()              # the CLI autotunes into the committed table: give it back as it was
    try:
        r = subprocess.run(["timeout", "-k", "10", "600", sys.executable, "-m", "adaptiveisp_amd.train", "--data", toy, "--augment",
                            "--iters", "2", "--batch", "2", "--size", "64"], cwd=ROOT, capture_output=True, text=True)
    finally:
        with open(cache, "wb") as f:
            f.write(saved)
    assert r.returncode == 0, r.stderr[-3000:]
    line = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1])
    assert line["data"].startswith("lod: 7 files, augment (hsv_h=0.015 "), line["data"]
    last = line["last"]
    assert np.isfinite([last["agent_loss"], last["value_loss"], last["reward"]]).all(), last
