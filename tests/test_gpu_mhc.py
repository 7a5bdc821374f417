"""The gradient-corrected (Malvar-He-Cutler) demosaic on the MI355X: adaisp_demosaic_ex and adaisp_demosaic_rects_ex
with ADAISP_DEMOSAIC_MHC (csrc/isp_demosaic.hip) against the float64 restatement (tests/_mhcref.py), bit for bit: whole
frames of one tile and of three tiles each way, rectangles on both store paths (zero outside, degenerate images all
zero), method 0 against the existing entries, ImageFolderSource(demosaic="mhc") and the two command lines. Every sum of
the filters is exact in fp32 (whole-number levels), so the restatement leaves no tolerance to choose."""
import json
import os
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

import _mhcref as M
import _unprocessref as U
from adaptiveisp_amd import _lib
from adaptiveisp_amd.data import ImageFolderSource
from adaptiveisp_amd.val.loader import load_letterboxed
from test_gpu_bayer import _rects, _stage, _u16

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
PATTERNS = ("RGGB", "GRBG", "GBRG", "BGGR")
LEVELS = [(64, 4095), (0, 65535)]                                  # (black, white), whole numbers: the sums are exact
# one tile; a tile edge the 2-pixel ring crosses (36 x 132 is the staged tile itself); three tiles each way
FRAMES = [(2, 2), (4, 6), (36, 132), (66, 258)]
# (h, w, S, top, left): odd sizes in an odd frame; the double fold; a 2-pixel side at the frame's edge; four tiles' corner;
# a rectangle one pixel past a tile each way; the whole frame
RECTS = [(5, 7, 37, 3, 5), (2, 2, 8, 1, 1), (2, 9, 16, 0, 3), (5, 5, 160, 30, 126), (33, 129, 192, 31, 1), (64, 64, 64, 0, 0)]


def _plane(rs, shape, black, white):
    """Seeded uint16 samples, below black and above white included."""
    hi = 65536 if white == 65535 else white + 105
    return rs.randint(0, hi, size=shape).astype(np.uint16)


def _dev(plane):
    return torch.from_numpy(plane.view(np.int16)).to(DEV)


def _out(B, S_or_hw, misalign=0):
    """A NaN-filled [B,3,H,W] view `misalign` floats into its buffer, sentinels before and after it."""
    H, W = (S_or_hw, S_or_hw) if isinstance(S_or_hw, int) else S_or_hw
    n = B * 3 * H * W
    buf = torch.full((misalign + n + 1024,), float("nan"), device=DEV)
    buf[:misalign] = 1234.5
    buf[misalign + n:] = -777.0
    return buf, buf[misalign:misalign + n].view(B, 3, H, W)


def _guards_intact(buf, out, misalign):
    b = buf.cpu()
    return bool((b[:misalign] == 1234.5).all() and (b[misalign + out.numel():] == -777.0).all())


# ------------------------------------------------------------------------------------------------------------ whole frame
@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("H,W", FRAMES)
def test_whole_frame_is_the_restatement(H, W, B):
    rs = np.random.RandomState(1000 * H + W + B)
    for black, white in LEVELS:
        plane = _plane(rs, (B, H, W), black, white)
        raw = _dev(plane)
        for pattern in PATTERNS:
            buf, out = _out(B, (H, W))
            got = _lib.demosaic(raw, pattern=pattern, black_level=black, white_level=white, out=out, method="mhc")
            assert got.data_ptr() == out.data_ptr() and _guards_intact(buf, out, 0)
            got = got.cpu().numpy()
            for b in range(B):
                want = M.mhc(plane[b], pattern, black, white)
                assert np.array_equal(got[b], want), (pattern, black, b, int((got[b] != want).sum()))


# ------------------------------------------------------------------------------------------------------------ rectangles
@pytest.mark.parametrize("misalign", [0, 1])
@pytest.mark.parametrize("h,w,S,top,left", RECTS)
def test_rects_are_the_restatement_of_the_crop(h, w, S, top, left, misalign):
    rs = np.random.RandomState(77 * h + w + S)
    desc = _rects([(h, w), (h, w)], [(top, left), (top, left)])
    pad = np.ones((S, S), bool)
    pad[top:top + h, left:left + w] = False
    for black, white in LEVELS:
        plane = _plane(rs, (2, S, S), black, white)           # the pad holds samples too: nothing of it may get in
        raw = _dev(plane)
        for pattern in PATTERNS:
            buf, out = _out(2, S, misalign)
            assert (out.data_ptr() % 8 != 0) == bool(misalign)
            _lib.demosaic_rects(raw, desc, pattern=pattern, black_level=black, white_level=white, out=out, method="mhc")
            assert _guards_intact(buf, out, misalign)
            got = out.cpu().numpy()
            for b in range(2):
                want = M.mhc_rect(plane[b], h, w, top, left, pattern, black, white)
                assert np.array_equal(got[b], want), (pattern, black, b, int((got[b] != want).sum()))
                assert (got[b][:, pad] == 0).all()
            if (h, w) == (S, S) and not misalign:
                whole = _lib.demosaic(raw, pattern=pattern, black_level=black, white_level=white, method="mhc")
                assert np.array_equal(whole.cpu().numpy(), got), pattern


def test_mixed_batch_of_eight_with_odd_offsets():
    S = 96
    dims = [(96, 96), (2, 2), (95, 3), (3, 95), (50, 77), (1, 40), (13, 96), (10, 10)]
    place = [(0, 0), (94, 93), (1, 47), (46, 1), (23, 9), (9, 23), (41, 0), (S - 9, 0)]    # the last one overhangs the frame
    desc = _rects(dims, place)
    rs = np.random.RandomState(8)
    for black, white in LEVELS:
        plane = _plane(rs, (8, S, S), black, white)
        raw = _dev(plane)
        for pattern in PATTERNS:
            buf, out = _out(8, S)
            _lib.demosaic_rects(raw, desc, pattern=pattern, black_level=black, white_level=white, out=out, method="mhc")
            got = out.cpu().numpy()
            assert _guards_intact(buf, out, 0) and np.isfinite(got).all()
            for b in range(8):
                (h, w), (top, left) = dims[b], place[b]
                want = M.mhc_rect(plane[b], h, w, top, left, pattern, black, white)
                assert np.array_equal(got[b], want), (pattern, b, int((got[b] != want).sum()))
                if b in (5, 7):
                    assert not got[b].any()                       # h = 1; a placement that does not fit
                else:
                    pad = np.ones((S, S), bool)
                    pad[top:top + h, left:left + w] = False
                    assert (got[b][:, pad] == 0).all() and got[b][:, ~pad].any()


# ------------------------------------------------------------------------------------------------------------ method 0
def test_method_bilinear_is_the_existing_entries():
    L = _lib.load()
    rs = np.random.RandomState(3)
    for (H, W), B in (((66, 258), 2), ((4, 6), 1)):
        raw = _dev(_plane(rs, (B, H, W), 64, 4095))
        for pat in range(4):
            old = torch.full((B, 3, H, W), float("nan"), device=DEV)
            assert L.adaisp_demosaic(raw.data_ptr(), old.data_ptr(), B, H, W, pat, 64.0, 4095.0, None) == 0
            new = _lib.demosaic(raw, pattern=pat, black_level=64, white_level=4095, method="bilinear")
            assert torch.equal(old.cpu(), new.cpu()) and torch.equal(
                new.cpu(), _lib.demosaic(raw, pattern=pat, black_level=64, white_level=4095).cpu())
    for h, w, S, top, left in RECTS:
        raw = _dev(_plane(rs, (2, S, S), 64, 4095))
        desc = _rects([(h, w), (h, w)], [(top, left), (top, left)])
        for pat in range(4):
            old = torch.full((2, 3, S, S), float("nan"), device=DEV)
            assert L.adaisp_demosaic_rects(raw.data_ptr(), desc.data_ptr(), old.data_ptr(), 2, S, pat, 64.0, 4095.0, None) == 0
            new = _lib.demosaic_rects(raw, desc, pattern=pat, black_level=64, white_level=4095, method="bilinear")
            assert torch.equal(old.cpu(), new.cpu())
            if h > 2 and w > 2:
                mhc = _lib.demosaic_rects(raw, desc, pattern=pat, black_level=64, white_level=4095, method="mhc")
                assert not torch.equal(mhc.cpu(), new.cpu())


def test_bad_methods_are_refused_on_the_device():
    raw = torch.zeros((1, 8, 8), dtype=torch.int16, device=DEV)
    desc = _rects([(4, 4)], [(0, 0)])
    out = torch.zeros((1, 3, 8, 8), device=DEV)
    L = _lib.load()
    for m in (-1, 2):
        assert L.adaisp_demosaic_ex(raw.data_ptr(), out.data_ptr(), 1, 8, 8, 0, m, 0.0, 1023.0, None) == -1
        assert L.adaisp_demosaic_rects_ex(raw.data_ptr(), desc.data_ptr(), out.data_ptr(), 1, 8, 0, m, 0.0, 1023.0, None) == -1
    with pytest.raises(_lib.AdaispError, match="method"):
        _lib.demosaic(raw, method="nope")
    with pytest.raises(_lib.AdaispError, match="method"):
        _lib.demosaic_rects(raw, desc, method="nope")
    for kw in (dict(pattern=4), dict(black_level=5, white_level=4)):
        with pytest.raises(_lib.AdaispError):
            _lib.demosaic(raw, method="mhc", **kw)
        with pytest.raises(_lib.AdaispError):
            _lib.demosaic_rects(raw, desc, method="mhc", **kw)


# ------------------------------------------------------------------------------------------------------------ the source
@pytest.fixture(scope="module")
def dataset(tmp_path_factory):
    root = tmp_path_factory.mktemp("mhcds")
    return str(root), U.write_dataset(str(root), [(12, 10), (9, 14)], seed=1)


def test_source_composes_the_sensor_and_the_mhc_demosaic(dataset):
    root, _ = dataset
    S = 64
    batch, plane = {}, {}
    for dm in ("bilinear", "mhc"):
        src = ImageFolderSource(root, S, DEV, sensor="bayer", demosaic=dm, workers=0, seed=2)
        try:
            ims, _, paths, _ = src.get_next_batch(2)
            batch[dm], plane[dm] = torch.stack(ims).cpu().numpy(), _u16(src._plane[:2])
            text = src.describe()
        finally:
            src.close()
        assert text == "lod: 2 files, bayer RGGB 12-bit black 64" + (", mhc demosaic" if dm == "mhc" else "")
    assert np.array_equal(plane["mhc"], plane["bilinear"])                   # one seed, one plane
    loaded = [load_letterboxed(p, S) for p in paths]
    src, desc = _stage([it[0] for it in loaded], [it[1] for it in loaded])
    raw = _lib.unprocess_bayer(src, desc, S, pattern="RGGB", black_level=64, white_level=4095)
    assert np.array_equal(_u16(raw), plane["mhc"])
    for dm in ("bilinear", "mhc"):
        want = _lib.demosaic_rects(raw, desc, black_level=64, white_level=4095, method=dm).cpu().numpy()
        assert np.array_equal(batch[dm], want), dm
    assert not np.array_equal(batch["mhc"], batch["bilinear"])
    for b, it in enumerate(loaded):                                           # and the restatement, through the whole path
        (h, w), (top, left) = it[0].shape[:2], it[1]
        assert np.array_equal(batch["mhc"][b], M.mhc_rect(plane["mhc"][b], h, w, top, left, "RGGB", 64, 4095))


def test_cli_trains_through_the_mhc_demosaic(dataset):
    root, _ = dataset
    cache = os.path.join(ROOT, "adaptiveisp_amd", "yolo", "tuning", "mi355x.json")
    saved = open(cache, "rb").read()              # the CLI autotunes into the committed table: give it back as it was
    try:
        r = subprocess.run(["timeout", "-k", "10", "600", sys.executable, "-m", "adaptiveisp_amd.train", "--data", root,
                            "--data-name", "coco", "--add-noise", "--sensor", "bayer", "--demosaic", "mhc", "--iters", "2",
                            "--batch", "2", "--size", "64"], cwd=ROOT, capture_output=True, text=True)
    finally:
        with open(cache, "wb") as f:
            f.write(saved)
    assert r.returncode == 0, r.stderr[-3000:]
    line = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1])
    assert line["data"] == "coco (unprocess, noise): 2 files, bayer RGGB 12-bit black 64, mhc demosaic", line["data"]
    last = line["last"]
    assert np.isfinite([last["agent_loss"], last["value_loss"], last["reward"]]).all(), last


def test_cli_val_through_the_mhc_demosaic(dataset, tmp_path):
    from test_gpu_val_cli import _agent_ckpt
    root, files = dataset
    with open(tmp_path / "two.txt", "w") as f:
        f.write("\n".join(files) + "\n")
    _agent_ckpt(tmp_path / "agent.pth")
    cmd = ["timeout", "-k", "10", "600", sys.executable, "-m", "adaptiveisp_amd.val", "--isp-ckpt", str(tmp_path / "agent.pth"),
           "--detector-ckpt", os.path.join(GOLD, "yolov3_w0625_refpickle.pt"), "--data", str(tmp_path / "two.txt"),
           "--data-name", "coco", "--add-noise", "--img-size", "64", "--batch-size", "2", "--project", str(tmp_path / "runs"),
           "--name", "mhc", "--sensor", "bayer", "--demosaic", "mhc"]
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    r = subprocess.run(cmd, cwd=ROOT, env=env, capture_output=True, text=True)
    assert r.returncode == 0, f"exit {r.returncode}\n{r.stdout[-3000:]}\n{r.stderr[-3000:]}"
    run = Path(r.stdout.strip().splitlines()[-1].split("Results saved to ", 1)[1])
    res = json.load(open(run / "results.json"))
    assert res["seen"] == 2 and res["args"]["sensor"] == "bayer" and res["args"]["demosaic"] == "mhc"
    assert np.isfinite([res[k] for k in ("mp", "mr", "map50", "map75", "map", "ms_per_image")]).all(), res
    rows = open(run / "records.txt").read().strip().splitlines()[1:]      # a header, then one row per image
    assert len(rows) == 2, rows
