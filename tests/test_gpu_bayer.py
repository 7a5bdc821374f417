"""The simulated Bayer sensor on the MI355X: adaisp_unprocess_bayer (csrc/isp_sensor.hip) as adaisp_unprocess sampled and
quantised, bit for bit, and against the reference's fixture (tests/golden/bayer.npz); adaisp_demosaic_rects
(csrc/isp_demosaic.hip) against the C oracle inside every rectangle, bit for bit, and zero outside; the pair on constant
colours at odd placements (no fringe, right phase); output bounds; the noise keys; ImageFolderSource(sensor="bayer") and
the two command lines."""
import json
import os
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

import _bayerref as R
import _unprocessref as U
from adaptiveisp_amd import _lib
from adaptiveisp_amd.data import ImageFolderSource, kernel_params, sample_unprocess_params
from adaptiveisp_amd.val.loader import load_letterboxed

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
# |fp32 kernel - float64 restatement| of the noise-free unprocess: the constants tests/test_gpu_unprocess.py records for
# this arithmetic (4x the largest error measured on the MI355X; the saturation case apart, where the mask's
# (gray - 0.9) / 0.1 amplifies the fp32 rounding of the colour matrix). The sensor adds the quantiser's half step.
TOL = 4 * 1.64e-7
TOL_SAT = 4 * 1.02e-6
NF = _lib.UNP_UNPROCESS | _lib.UNP_NOISE
PATTERNS = ("RGGB", "GRBG", "GBRG", "BGGR")
LEVELS = [(10, 64), (12, 256), (16, 0)]                   # (raw_bits, black)
# (h, w, S, top, left): 8-byte and per-sample stores, odd placement, odd sizes, one tile and several
SHAPES = [(2, 2, 2, 0, 0), (2, 2, 8, 3, 5), (3, 5, 7, 1, 1), (29, 33, 37, 3, 1), (37, 511, 512, 237, 0),
          (512, 512, 512, 0, 0)]


def _u16(t):
    """A uint16 / int16 device tensor as a uint16 numpy array."""
    return t.view(torch.int16).cpu().numpy().view(np.uint16)


def _stage(imgs, place, params=None, serials=None, gap=0):
    """uint8 HWC BGR arrays at (top, left) each, `gap` bytes between them -> (src bytes, descriptor bytes) on the device."""
    desc = np.zeros(len(imgs), _lib.UNPROCESS_DESC)
    chunks, off = [], gap
    for b, im in enumerate(imgs):
        chunks += [np.full(gap, 77, np.uint8), im.reshape(-1)]
        desc[b]["src_offset"], desc[b]["h"], desc[b]["w"] = off, im.shape[0], im.shape[1]
        desc[b]["top"], desc[b]["left"] = place[b]
        desc[b]["serial"] = b if serials is None else serials[b]
        if params is not None:
            desc[b]["p"] = params[b]
        off += gap + im.size
    src = torch.from_numpy(np.concatenate(chunks + [np.full(gap, 77, np.uint8)])).to(DEV)
    return src, torch.from_numpy(desc.view(np.uint8).copy()).to(DEV)


def _rects(imgs, place):
    """Descriptors alone (what adaisp_demosaic_rects reads of them: the rectangles)."""
    return _stage([np.zeros((h, w, 3), np.uint8) for h, w in imgs], place)[1]


def _rand_u8(rs, h, w, lo=0, hi=256):
    im = rs.randint(lo, hi, size=(h, w, 3)).astype(np.uint8)
    if lo == 0 and hi == 256:
        im.reshape(-1)[0], im.reshape(-1)[-1] = 0, 255
    return im


def _params(seed, noise=False, bri=None):
    return kernel_params(sample_unprocess_params(np.random.RandomState(seed), noise, bri))


def _expected_plane(u, dims, place, pattern, black, white):
    """[S,S] uint16 from the fp32 [3,S,S] output `u` of adaisp_unprocess: the CFA channel of every pixel of the image,
    quantised with the kernel's two fp32 operations; black around it."""
    (h, w), (top, left) = dims, place
    S = u.shape[-1]
    out = np.full((S, S), black, np.uint16)
    if h and w and top >= 0 and left >= 0 and top + h <= S and left + w <= S:
        ch = R.cfa_channels(h, w, pattern)
        v = np.take_along_axis(u[:, top:top + h, left:left + w], ch[None], axis=0)[0]
        assert v.dtype == np.float32
        out[top:top + h, left:left + w] = R.quantise(v, black, white)
    return out


# ------------------------------------------------------------------------------------------------------------ the sensor
@pytest.mark.parametrize("flags", [0, _lib.UNP_UNPROCESS, NF])
@pytest.mark.parametrize("h,w,S,top,left", SHAPES)
def test_sensor_is_unprocess_sampled_and_quantised(h, w, S, top, left, flags):
    rs = np.random.RandomState(h * 1000 + w)
    im = _rand_u8(rs, h, w)
    src, desc = _stage([im], [(top, left)], [_params(h + w, noise=True, bri=(0.3, 0.9))], serials=[h + 3], gap=(w % 2) + 1)
    u = _lib.unprocess(src, desc, S, seed=11, flags=flags).cpu().numpy()[0]
    for pattern in PATTERNS:
        for bits, black in LEVELS:
            white = 2 ** bits - 1
            got = _u16(_lib.unprocess_bayer(src, desc, S, seed=11, flags=flags, pattern=pattern, black_level=black,
                                            white_level=white))[0]
            want = _expected_plane(u, (h, w), (top, left), pattern, black, white)
            assert np.array_equal(got, want), (pattern, bits, int((got != want).sum()))
            pad = np.ones((S, S), bool)
            pad[top:top + h, left:left + w] = False
            assert (got[pad] == black).all()


def test_sensor_mixed_batch_of_eight_with_odd_offsets():
    rs = np.random.RandomState(8)
    S = 96
    dims = [(96, 96), (2, 2), (95, 3), (3, 95), (50, 77), (77, 50), (13, 96), (96, 13)]
    place = [(0, 0), (94, 93), (1, 47), (46, 1), (23, 9), (9, 23), (41, 0), (0, 41)]
    imgs = [_rand_u8(rs, h, w) for h, w in dims]
    src, desc = _stage(imgs, place, [_params(20 + b, noise=True, bri=(0.1, 0.3)) for b in range(8)], gap=7)
    for flags, pattern in ((0, "RGGB"), (_lib.UNP_UNPROCESS, "GBRG"), (NF, "GRBG")):
        u = _lib.unprocess(src, desc, S, seed=5, flags=flags).cpu().numpy()
        got = _u16(_lib.unprocess_bayer(src, desc, S, seed=5, flags=flags, pattern=pattern, black_level=64, white_level=4095))
        for b in range(8):
            assert np.array_equal(got[b], _expected_plane(u[b], dims[b], place[b], pattern, 64, 4095)), (flags, b)


def test_sensor_matches_reference_fixture(golden):
    """|plane / 65535 - reference| <= half a quantisation step + the recorded fp32 error of the shared arithmetic."""
    z = golden("bayer")
    cases = [f"case{k}." for k in range(64) if f"case{k}.plane" in z.files]
    assert len(cases) >= 6
    assert (U.saturation_mask(z["sat.img"], z["sat.rgb2cam"]) > 0.05).sum() >= 10
    for c in cases + ["sat."]:
        img, g = z[c + "img"], z[c + "gains"]
        m = dict(rgb2cam=z[c + "rgb2cam"], rgb_gain=g[0], red_gain=g[1], blue_gain=g[2], gain=1.0, shot=0.0, read=0.0)
        h, w = img.shape[:2]
        S = max(h, w) + 3
        src, desc = _stage([img], [(1, 3)], [kernel_params(m, 1.0)], gap=1)
        got = _u16(_lib.unprocess_bayer(src, desc, S, flags=_lib.UNP_UNPROCESS, pattern="RGGB", black_level=0,
                                        white_level=65535))[0]
        err = np.abs(got[1:1 + h, 3:3 + w] / 65535.0 - z[c + "plane"]).max()
        print(f"bayer fixture {c} max |plane / 65535 - ref| = {err:.3e}")
        assert err <= 0.5 / 65535 + (TOL_SAT if c == "sat." else TOL), (c, err)


# ------------------------------------------------------------------------------------------------------------ the demosaic
@pytest.mark.parametrize("h,w,S,top,left", SHAPES)
def test_rect_demosaic_is_the_oracle_of_the_crop(oracle_mod, h, w, S, top, left):
    rs = np.random.RandomState(h * 77 + w)
    plane = rs.randint(0, 4200, size=(2, S, S)).astype(np.uint16)       # below black and above white included
    raw = torch.from_numpy(plane.view(np.int16)).to(DEV)
    desc = _rects([(h, w), (h, w)], [(top, left), (top, left)])
    for pattern in PATTERNS:
        got = _lib.demosaic_rects(raw, desc, pattern=pattern, black_level=64, white_level=4095).cpu().numpy()
        for b in range(2):
            want = R.demosaic_rect(plane[b], h, w, top, left, pattern, 64, 4095)
            assert np.array_equal(got[b], want), (pattern, b, int((got[b] != want).sum()))
            pad = np.ones((S, S), bool)
            pad[top:top + h, left:left + w] = False
            assert (got[b][:, pad] == 0).all()
        if (h, w) == (S, S) and S % 2 == 0:
            whole = _lib.demosaic(raw, pattern=pattern, black_level=64, white_level=4095)
            assert torch.equal(whole.cpu(), torch.from_numpy(got)), pattern


@pytest.mark.parametrize("h,w", [(6, 8), (5, 7)])
@pytest.mark.parametrize("pattern", PATTERNS)
def test_no_fringe_and_right_phase_on_a_constant_colour(h, w, pattern):
    S, top, left, black, white = 16, 3, 5, 64, 4095
    bgr = np.array([30, 200, 117], np.uint8)
    im = np.broadcast_to(bgr, (h, w, 3)).copy()
    src, desc = _stage([im], [(top, left)], gap=1)
    raw = _lib.unprocess_bayer(src, desc, S, pattern=pattern, black_level=black, white_level=white)
    got = _lib.demosaic_rects(raw, desc, pattern=pattern, black_level=black, white_level=white).cpu().numpy()[0]
    q = R.quantise(bgr[::-1].astype(np.float32) / np.float32(255), black, white).astype(np.float32)
    rgb = (q - np.float32(black)) * (np.float32(1) / np.float32(white - black))
    want = np.zeros((3, S, S), np.float32)
    want[:, top:top + h, left:left + w] = rgb[:, None, None]
    assert np.array_equal(got, want), np.argwhere(got != want)[:8]


# ------------------------------------------------------------------------------------------------------------ bounds
@pytest.mark.parametrize("S,misalign", [(64, 0), (64, 1), (37, 0), (37, 1)])
def test_bounds_pad_and_degenerate_images(S, misalign):
    """Sentinels around [B,S,S] / [B,3,S,S] (and before a start one element off: the per-sample store paths) stay as they
    were; a placement that does not fit and an image of one row come out all black / all zero."""
    rs = np.random.RandomState(S)
    imgs = [_rand_u8(rs, 20, S), _rand_u8(rs, S, 9), _rand_u8(rs, 1, 6), _rand_u8(rs, 10, 10)]
    place = [(5, 0), (0, S - 9), (S - 1, 3), (S - 9, 0)]                 # the last one overhangs the frame
    B, black, white = 4, 64, 1023
    src, desc = _stage(imgs, place, [_params(b, noise=True) for b in range(B)], gap=3)
    n = B * S * S
    sent = np.array([0xA5A5], np.uint16).view(np.int16)[0]
    pbuf = torch.full((n + 4096 + misalign,), int(sent), dtype=torch.int16, device=DEV)
    plane = pbuf[misalign:misalign + n].view(B, S, S)
    obuf = torch.full((3 * n + 4096 + misalign,), float("nan"), device=DEV)
    obuf[:misalign] = 1234.5
    obuf[misalign + 3 * n:] = -777.0
    out = obuf[misalign:misalign + 3 * n].view(B, 3, S, S)
    for flags in (0, _lib.UNP_UNPROCESS, NF):
        _lib.unprocess_bayer(src, desc, S, seed=2, flags=flags, pattern="GBRG", black_level=black, white_level=white,
                             out=plane)
        _lib.demosaic_rects(plane, desc, pattern="GBRG", black_level=black, white_level=white, out=out)
        p = _u16(pbuf)
        assert (p[:misalign] == 0xA5A5).all() and (p[misalign + n:] == 0xA5A5).all()
        p = p[misalign:misalign + n].reshape(B, S, S)
        assert (p <= white).all()
        o = obuf.cpu()
        assert (o[:misalign] == 1234.5).all() and (o[misalign + 3 * n:] == -777.0).all()
        o = out.cpu().numpy()
        assert np.isfinite(o).all()
        for b in range(2):
            pad = np.ones((S, S), bool)
            pad[place[b][0]:place[b][0] + imgs[b].shape[0], place[b][1]:place[b][1] + imgs[b].shape[1]] = False
            assert (p[b][pad] == black).all() and (o[b][:, pad] == 0).all() and (p[b][~pad] != black).any()
            want = R.demosaic_rect(p[b], *imgs[b].shape[:2], *place[b], "GBRG", black, white)
            assert np.array_equal(o[b], want), b
        # h = 1: the sensor still samples its row, the demosaic has nothing to mirror onto
        row = p[2][S - 1, 3:9].copy()
        p[2][S - 1, 3:9] = black
        assert (row != black).any() and (p[2] == black).all() and (o[2] == 0).all()
        assert (p[3] == black).all() and (o[3] == 0).all()


def test_bad_arguments_are_refused():
    src, desc = _stage([np.zeros((4, 4, 3), np.uint8)], [(0, 0)])
    raw = torch.zeros((1, 8, 8), dtype=torch.int16, device=DEV)
    for kw in (dict(pattern=4), dict(pattern=-1), dict(black_level=1023, white_level=1023), dict(black_level=5, white_level=4),
               dict(flags=_lib.UNP_NOISE), dict(flags=8)):
        with pytest.raises(_lib.AdaispError):
            _lib.unprocess_bayer(src, desc, 8, **kw)
        if "flags" not in kw:
            with pytest.raises(_lib.AdaispError):
                _lib.demosaic_rects(raw, desc, **kw)
    with pytest.raises(_lib.AdaispError):
        _lib.demosaic_rects(raw, torch.cat([desc, desc]))                 # two descriptors, one plane
    with pytest.raises(_lib.AdaispError):
        _lib.demosaic_rects(raw.float(), desc)
    with pytest.raises(_lib.AdaispError):
        _lib.unprocess_bayer(src, desc, 8, out=torch.zeros((1, 8, 8), device=DEV))
    with pytest.raises(_lib.AdaispError):
        _lib.unprocess_bayer(src.cpu(), desc, 8)
    L = _lib.load()
    assert L.adaisp_unprocess_bayer(None, desc.data_ptr(), raw.data_ptr(), 1, 8, 0, 0, 0, 0.0, 1023.0, None) == -1
    assert L.adaisp_demosaic_rects(raw.data_ptr(), None, raw.data_ptr(), 1, 8, 0, 0.0, 1023.0, None) == -1
    assert L.adaisp_demosaic_rects(raw.data_ptr(), desc.data_ptr(), raw.data_ptr(), 65536, 8, 0, 0.0, 1023.0, None) == -4
    assert L.adaisp_unprocess_bayer(src.data_ptr(), desc.data_ptr(), raw.data_ptr(), 1, 32769, 0, 0, 0, 0.0, 1023.0, None) == -4


# ------------------------------------------------------------------------------------------------------------ noise keys
def test_plane_is_a_function_of_seed_and_serial():
    rs = np.random.RandomState(5)
    imgs = [_rand_u8(rs, 60, 70, 120, 256) for _ in range(8)]
    params = []
    for b in range(8):
        p = _params(b)
        p[14], p[15] = 0.001, 1e-5
        params.append(p)
    place = [(b, b + 1) for b in range(8)]
    kw = dict(flags=NF, pattern="GRBG", black_level=64, white_level=4095)
    src, desc = _stage(imgs, place, params, serials=list(range(100, 108)), gap=3)
    a = _u16(_lib.unprocess_bayer(src, desc, 80, seed=7, **kw))
    assert np.array_equal(a, _u16(_lib.unprocess_bayer(src, desc, 80, seed=7, **kw)))
    # image 5 alone: another batch slot, byte offset, frame size and (odd / even swapped) placement, the same samples
    s1, d1 = _stage([imgs[5]], [(2, 1)], [params[5]], serials=[105], gap=0)
    alone = _u16(_lib.unprocess_bayer(s1, d1, 73, seed=7, **kw))[0]
    t, l = place[5]
    assert np.array_equal(alone[2:62, 1:71], a[5, t:t + 60, l:l + 70])
    other = _u16(_lib.unprocess_bayer(s1, _stage([imgs[5]], [(2, 1)], [params[5]], serials=[106])[1], 73, seed=7, **kw))[0]
    assert (other[2:62, 1:71] != alone[2:62, 1:71]).mean() > 0.5
    assert (_u16(_lib.unprocess_bayer(s1, d1, 73, seed=8, **kw))[0][2:62, 1:71] != alone[2:62, 1:71]).mean() > 0.5
    assert np.array_equal(other[0], np.full(73, 64, np.uint16))


# ------------------------------------------------------------------------------------------------------------ the source
SIZES = [(40, 30), (17, 50), (64, 64), (33, 21), (80, 12), (9, 71), (25, 25), (130, 90), (3, 3)]   # odd sides; 130 x 90 and
#                                                                                  80 x 12 overshoot load_image's ceil at 64


@pytest.fixture(scope="module")
def dataset(tmp_path_factory):
    root = tmp_path_factory.mktemp("bayerds")
    return str(root), U.write_dataset(str(root), SIZES, seed=9, nc=7)


def _batches(root, counts=(4, 5), **kw):
    src = ImageFolderSource(root, 64, DEV, **kw)
    try:
        out, paths = [], []
        for n in counts:
            ims, _, p, _ = src.get_next_batch(n)
            out.append(torch.stack(ims).cpu())
            paths += p
        return torch.cat(out).numpy(), paths, src.describe()
    finally:
        src.close()


def test_bayer_source_composes_the_two_kernels(dataset):
    root, _ = dataset
    S, kw = 64, dict(data_name="coco", add_noise=True, brightness_range=(0.2, 0.6), seed=4)
    got, paths, text = _batches(root, workers=0, sensor="bayer", cfa="GRBG", raw_bits=10, **kw)
    assert text == "coco (unprocess, noise): 9 files, bayer GRBG 10-bit black 16"
    assert got.shape == (9, 3, S, S) and np.isfinite(got).all()
    # by hand, on load_letterboxed's images, with the source's metadata draws, serials and seed
    rs = np.random.RandomState(4000)
    done = 0
    for n in (4, 5):
        loaded = [load_letterboxed(p, S) for p in paths[done:done + n]]
        params = [kernel_params(sample_unprocess_params(rs, True, (0.2, 0.6))) for _ in range(n)]
        src, desc = _stage([it[0] for it in loaded], [it[1] for it in loaded], params, serials=list(range(done, done + n)))
        raw = _lib.unprocess_bayer(src, desc, S, seed=4000, flags=NF, pattern="GRBG", black_level=16, white_level=1023)
        want = _lib.demosaic_rects(raw, desc, pattern="GRBG", black_level=16, white_level=1023).cpu().numpy()
        assert np.array_equal(got[done:done + n], want)
        done += n
    # the decoding threads and the device resample change nothing
    assert np.array_equal(_batches(root, workers=4, sensor="bayer", cfa="GRBG", raw_bits=10, **kw)[0], got)
    dev, _, text = _batches(root, workers=2, resize="device", sensor="bayer", cfa="GRBG", raw_bits=10, **kw)
    assert np.array_equal(dev, got) and text.endswith("device resize, bayer GRBG 10-bit black 16")
    # green at the green sites is the rgb batch's green, quantised: same parameters, same normals
    rgb = _batches(root, workers=0, **kw)[0]
    for b, path in enumerate(paths):
        u8, (top, left), *_ = load_letterboxed(path, S)
        h, w = u8.shape[:2]
        site = R.cfa_channels(h, w, "GRBG") == 1
        q = R.quantise(rgb[b, 1, top:top + h, left:left + w], 16, 1023).astype(np.float32)
        want = (q - np.float32(16)) * (np.float32(1) / np.float32(1023 - 16))
        assert np.array_equal(got[b, 1, top:top + h, left:left + w][site], want[site]), path


def test_bayer_source_on_lod_images_and_tiny_files(dataset, tmp_path):
    root, _ = dataset
    got, paths, text = _batches(root, counts=(3,), workers=0, sensor="bayer")
    assert text == "lod: 9 files, bayer RGGB 12-bit black 64"
    loaded = [load_letterboxed(p, 64) for p in paths]
    src, desc = _stage([it[0] for it in loaded], [it[1] for it in loaded])
    raw = _lib.unprocess_bayer(src, desc, 64, pattern="RGGB", black_level=64, white_level=4095)
    assert np.array_equal(got, _lib.demosaic_rects(raw, desc, black_level=64, white_level=4095).cpu().numpy())
    files = U.write_dataset(str(tmp_path), [(8, 8), (200, 2)], seed=3)      # 200 x 2 -> 64 x 1 at size 64
    src = ImageFolderSource(str(tmp_path), 64, DEV, sensor="bayer", workers=0)
    try:
        with pytest.raises(ValueError, match=os.path.basename(files[1])):
            src.get_next_batch(2)
    finally:
        src.close()


def test_cli_trains_through_the_sensor(dataset):
    root, _ = dataset
    cache = os.path.join(ROOT, "adaptiveisp_amd", "yolo", "tuning", "mi355x.json")
    saved = open(cache, "rb").read()              # the CLI autotunes into the committed table: give it back as it was
    try:
        r = subprocess.run(["timeout", "-k", "10", "600", sys.executable, "-m", "adaptiveisp_amd.train", "--data", root,
                            "--data-name", "coco", "--add-noise", "--sensor", "bayer", "--iters", "2", "--batch", "2",
                            "--size", "64"], cwd=ROOT, capture_output=True, text=True)
    finally:
        with open(cache, "wb") as f:
            f.write(saved)
    assert r.returncode == 0, r.stderr[-3000:]
    line = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1])
    assert line["data"] == "coco (unprocess, noise): 9 files, bayer RGGB 12-bit black 64", line["data"]
    last = line["last"]
    assert np.isfinite([last["agent_loss"], last["value_loss"], last["reward"]]).all(), last


def test_cli_val_through_the_sensor(dataset, tmp_path):
    from test_gpu_val_cli import _agent_ckpt
    root, files = dataset
    with open(tmp_path / "three.txt", "w") as f:
        f.write("\n".join(files[:3]) + "\n")
    _agent_ckpt(tmp_path / "agent.pth")
    cmd = ["timeout", "-k", "10", "600", sys.executable, "-m", "adaptiveisp_amd.val", "--isp-ckpt", str(tmp_path / "agent.pth"),
           "--detector-ckpt", os.path.join(GOLD, "yolov3_w0625_refpickle.pt"), "--data", str(tmp_path / "three.txt"),
           "--data-name", "coco", "--add-noise", "--img-size", "64", "--batch-size", "2", "--project", str(tmp_path / "runs"),
           "--name", "bayer", "--sensor", "bayer", "--raw-bits", "10"]
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    r = subprocess.run(cmd, cwd=ROOT, env=env, capture_output=True, text=True)
    assert r.returncode == 0, f"exit {r.returncode}\n{r.stdout[-3000:]}\n{r.stderr[-3000:]}"
    run = Path(r.stdout.strip().splitlines()[-1].split("Results saved to ", 1)[1])
    res = json.load(open(run / "results.json"))
    assert res["seen"] == 3 and res["args"]["sensor"] == "bayer" and res["args"]["raw_bits"] == 10
    rows = open(run / "records.txt").read().strip().splitlines()[1:]      # a header, then one row per image
    assert len(rows) == 3, rows
