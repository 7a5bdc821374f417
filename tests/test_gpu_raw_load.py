"""adaisp_raw_load on the MI355X (csrc/isp_raw_load.hip): native-size uint16 colour-filter-array planes -> the letterboxed
fp32 batch in one launch, against the numpy definition (tests/_rawref.py) bit for bit: every comparison is np.array_equal
on the uint32 view of the output, and `out` is pre-filled with NaN between guard words, so an unwritten sample and a write
outside `out` both show. Then the data source (ImageFolderSource(data_name="raw")) and the evaluation command line on
.npy planes."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import _rawref as R
from adaptiveisp_amd import _lib
from adaptiveisp_amd.resize import RawTapPlan, _csr, raw_table

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PATTERNS = ("RGGB", "GRBG", "GBRG", "BGGR")
METHODS = ("bilinear", "mhc")
LEVELS = [(0, 4095), (64, 4095), (0, 65535), (64, 65535)]            # (black, white)
# (H, W) -> (h, w). The kernel's tile: a workgroup owns 4 frame rows (RL_ROWS) and walks groups of at most 128 output
# columns (RL_THREADS), whose staged source span holds at most 1280 columns (RL_CW) whatever the factor.
SHAPES = [
    ((2, 2), (2, 2)), ((7, 9), (4, 5)), ((37, 53), (16, 23)), ((64, 96), (16, 24)), ((300, 520), (20, 35)),
    ((10, 14), (23, 32)), ((33, 47), (17, 24)),
    ((40, 150), (17, 65)), ((70, 300), (33, 129)),                    # widths 65, 129; heights 17, 33
    ((12, 140), (5, 129)),                                            # one more than the tile: 4 rows, 128 columns
    ((20, 40), (33, 65)),                                             # enlarging across a row band and a column group
    ((101, 300), (100, 297)),                                         # shrinking by 1.01: three groups of 99 columns
    ((60, 1350), (2, 45)),                                            # shrinking by 30: the span bounds the group (42 columns)
    ((9, 2600), (9, 2600 // 2)),                                      # 1300 columns: groups of 128 whose spans tile the row
]


def _stage(planes, specs, gains=None, offsets=None, tables=None):
    """The device buffers of one call: (src bytes, desc bytes, tabs int32, host records). specs: ((h, w), (top, left)) per
    plane; planes start 16-byte aligned unless `offsets` says otherwise; tables: {b: (tx, ty)} custom CSR tables."""
    plan = RawTapPlan()
    pos, offs = 0, []
    for b, p in enumerate(planes):
        off = pos if offsets is None else offsets[b]
        offs.append(off)
        pos = (off + p.nbytes + 15) // 16 * 16
    src = np.zeros(pos + 16, np.uint8)
    for b, (p, (hw, place)) in enumerate(zip(planes, specs)):
        src[offs[b]:offs[b] + p.nbytes] = p.reshape(-1).view(np.uint8)
        plan.add(p.shape if p.ndim == 2 and min(p.shape) >= 1 else (1, 1), hw, place, offs[b],
                 (1.0, 1.0, 1.0) if gains is None else gains[b])
    rec, tab = plan.descriptors(), plan.table()
    for b, (tx, ty) in (tables or {}).items():
        rec[b]["tab_x"], rec[b]["tab_y"] = tab.size, tab.size + tx.size
        tab = np.concatenate([tab, tx, ty])
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(DEV)
    return dev(src), dev(rec.view(np.uint8)), dev(tab.astype(np.int32)), rec


def _out(B, S):
    n = B * 3 * S * S
    buf = torch.full((n + 2048,), float("nan"), device=DEV)
    buf[:1024] = 1234.5
    buf[1024 + n:] = -777.0
    return buf, buf[1024:1024 + n].view(B, 3, S, S)


def _guards_intact(buf):
    b = buf.cpu()
    return bool((b[:1024] == 1234.5).all() and (b[-1024:] == -777.0).all())


def _same(got, want):
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want, dtype=np.float32)
    return got.shape == want.shape and np.array_equal(got.view(np.uint32), want.view(np.uint32))


def _load(src, desc, tabs, B, S, **kw):
    buf, out = _out(B, S)
    _lib.raw_load(src, desc, tabs, S, out=out, **kw)
    torch.cuda.synchronize()
    assert _guards_intact(buf)
    return out.cpu().numpy()


# ------------------------------------------------------------------------------------------------------------ shapes
@pytest.mark.parametrize("src_hw,dst_hw", SHAPES)
def test_shape_is_the_definition(src_hw, dst_hw):
    (H, W), (h, w) = src_hw, dst_hw
    S, place = max(h, w) + 3, (1, 2)
    rs = np.random.RandomState(1000 * H + W)
    smooth = R.plane(H, W, H + W)
    noisy = rs.randint(0, 65536, size=(H, W)).astype(np.uint16)       # samples below black and above white included
    src, desc, tabs, _ = _stage([smooth, noisy], [(dst_hw, place)] * 2)
    for black, white in LEVELS:
        for method in METHODS:
            for pattern in PATTERNS:
                got = _load(src, desc, tabs, 2, S, pattern=pattern, method=method, black_level=black, white_level=white)
                for b, p in enumerate((smooth, noisy)):
                    want = R.raw_load_one(p, dst_hw, place, S, pattern, method, black, white)
                    assert _same(got[b], want), (src_hw, dst_hw, black, white, method, pattern, b)


# ------------------------------------------------------------------------------------------------------------ gains
@pytest.mark.parametrize("method", METHODS)
def test_gains(method):
    p = R.plane(37, 53, 5)
    spec = [((16, 23), (3, 1))]
    src, desc, tabs, _ = _stage([p], spec, gains=[(1.9, 1.0, 1.6)])
    got = _load(src, desc, tabs, 1, 32, pattern="GBRG", method=method, black_level=64, white_level=4095)
    assert _same(got[0], R.raw_load_one(p, (16, 23), (3, 1), 32, "GBRG", method, 64, 4095, gains=(1.9, 1.0, 1.6)))
    src, desc, tabs, _ = _stage([p], spec, gains=[(1.0, 1.0, 1.0)])
    unit = _load(src, desc, tabs, 1, 32, pattern="GBRG", method=method, black_level=64, white_level=4095)
    assert _same(unit[0], R.raw_load_one(p, (16, 23), (3, 1), 32, "GBRG", method, 64, 4095, gains=None))
    assert not _same(unit[0], got[0])


# ------------------------------------------------------------------------------------------------------------ batch
@pytest.mark.parametrize("S", [33, 64])
@pytest.mark.parametrize("method", METHODS)
def test_batch_and_placement(S, method):
    """Mixed sizes in one call: odd top / left, a plane at an offset that is a multiple of 2 but not of 16, a placement that
    does not fit, a one-column plane."""
    planes = [R.plane(37, 53, 1), R.plane(10, 14, 2), R.plane(64, 96, 3), R.plane(20, 30, 4),
              np.full((9, 1), 700, np.uint16)]
    specs = [((16, 23), (1, 3)), ((23, 32), (5, 1)), ((16, 24), (17, 9)), ((10, 15), (S - 9, 0)), ((9, 1), (0, 0))]
    offsets, pos = [], 0
    for b, p in enumerate(planes):
        pos = (pos + 15) // 16 * 16 + (6 if b == 2 else 0)            # plane 2: 2-byte aligned only
        offsets.append(pos)
        pos += p.nbytes
    gains = [(1.0, 1.0, 1.0), (1.9, 1.0, 1.6), (0.5, 1.0, 2.0), (1.0, 1.0, 1.0), (1.0, 1.0, 1.0)]
    src, desc, tabs, _ = _stage(planes, specs, gains=gains, offsets=offsets)
    got = _load(src, desc, tabs, 5, S, pattern="GRBG", method=method, black_level=64, white_level=4095)
    for b, (p, (hw, place)) in enumerate(zip(planes, specs)):
        assert _same(got[b], R.raw_load_one(p, hw, place, S, "GRBG", method, 64, 4095, gains=gains[b])), b
    assert not got[3].any() and not got[4].any()                      # does not fit; src_w = 1
    assert got[0].any() and got[1].any() and got[2].any()


def test_odd_offset_is_zero():
    p = R.plane(8, 8, 1)
    src, desc, tabs, rec = _stage([p, p], [((4, 4), (0, 0))] * 2, offsets=[0, 129])
    got = _load(src, desc, tabs, 2, 8, method="mhc", black_level=64, white_level=4095)
    assert _same(got[0], R.raw_load_one(p, (4, 4), (0, 0), 8, "RGGB", "mhc", 64, 4095)) and not got[1].any()


# ------------------------------------------------------------------------------------------------------------ bounds
@pytest.mark.parametrize("method", METHODS)
def test_plane_or_taps_outside_their_buffers(method):
    """The last plane's last row past src_bytes; then the last image's taps past tab_words: that image all zero, the
    others right, nothing outside `out` written (the guards in _load)."""
    planes = [R.plane(37, 53, 1), R.plane(33, 47, 2), R.plane(64, 96, 3)]
    specs = [((16, 23), (0, 0)), ((17, 24), (2, 3)), ((16, 24), (1, 1))]
    src, desc, tabs, rec = _stage(planes, specs)
    want = [R.raw_load_one(p, hw, place, 32, "RGGB", method, 64, 4095) for p, (hw, place) in zip(planes, specs)]
    kw = dict(method=method, black_level=64, white_level=4095)
    end = int(rec[2]["src_offset"]) + planes[2].nbytes
    full = _load(src[:end], desc, tabs, 3, 32, **kw)
    assert all(_same(full[b], want[b]) for b in range(3))
    short = _load(src[:end - 2], desc, tabs, 3, 32, **kw)             # one sample short
    assert _same(short[0], want[0]) and _same(short[1], want[1]) and not short[2].any()
    fewer = _load(src, desc, tabs[:-1], 3, 32, **kw)                  # the last table (image 2's vertical taps) one word short
    assert _same(fewer[0], want[0]) and _same(fewer[1], want[1]) and not fewer[2].any()


# ------------------------------------------------------------------------------------------------------------ other taps
@pytest.mark.parametrize("method", METHODS)
def test_taps_that_are_not_the_hosts(method):
    """Any CSR table is computed as the contract says: taps out of source order and far apart (outside the span the kernel
    stages, so their neighbourhoods come from global memory), an index past the plane (clamped), an empty row."""
    H, W, h, w = 21, 40, 6, 7
    p = R.plane(H, W, 9)
    wx = np.float32([0.25, 0.5, 0.25])
    tx = _csr(np.full(w, 3), np.stack([W - 1 - 5 * np.arange(w), 5 * np.arange(w), np.full(w, W + 7)], 1).reshape(-1),
              np.tile(wx, w))
    ty = _csr(np.array([2, 0, 2, 2, 2, 2]), np.array([20, 0, 3, 4, 9, 2, 25, 10, 11, 12]),
              np.float32([0.5, 0.5, 1, 1, 0.3, 0.7, 0.5, 0.5, 0.1, 0.9]))
    src, desc, tabs, _ = _stage([p], [((h, w), (1, 1))], tables={0: (tx, ty)})
    got = _load(src, desc, tabs, 1, 9, pattern="BGGR", method=method, black_level=64, white_level=4095)
    cx, cy = tx.copy(), ty.copy()
    cx[w + 1:w + 1 + 3 * w] = np.minimum(cx[w + 1:w + 1 + 3 * w], W - 1)      # the reference clamps as the kernel does
    cy[h + 1:h + 1 + 10] = np.minimum(cy[h + 1:h + 1 + 10], H - 1)
    assert _same(got[0], R.raw_load_one(p, (h, w), (1, 1), 9, "BGGR", method, 64, 4095, tx=cx, ty=cy))


def test_argument_checks_on_the_device_side_of_the_binding():
    p = R.plane(8, 8, 1)
    src, desc, tabs, _ = _stage([p], [((4, 4), (0, 0))])
    with pytest.raises(_lib.AdaispError):
        _lib.raw_load(src.cpu(), desc, tabs, 8)
    with pytest.raises(_lib.AdaispError):
        _lib.raw_load(src, desc[:-1], tabs, 8)
    with pytest.raises(_lib.AdaispError):
        _lib.raw_load(src, desc, tabs, 8, method="nearest")
    with pytest.raises(_lib.AdaispError):
        _lib.raw_load(src, desc, tabs, 8, black_level=5.0, white_level=5.0)
    out = torch.zeros((1, 3, 8, 8), device=DEV)
    v = out._version
    _lib.raw_load(src, desc, tabs, 8, out=out)
    assert out._version > v


# ------------------------------------------------------------------------------------------------------------ the source
S_DATA = 256                                                          # the size and batch of tests/test_gpu_val_cli.py
SENSOR = dict(cfa="GRBG", raw_bits=12, demosaic="mhc", raw_gains=(1.9, 1.0, 1.6))      # black: the default, 64


@pytest.fixture(scope="module")
def planes_dir(tmp_path_factory):
    """Five planes of different native sizes (shrunk, kept and enlarged at 256) with YOLO labels beside them."""
    root = tmp_path_factory.mktemp("rawdata")
    os.makedirs(root / "images"), os.makedirs(root / "labels")
    rng = np.random.default_rng(21)
    for i, (h, w) in enumerate([(300, 400), (256, 192), (333, 250), (180, 320), (240, 240)]):
        stem = "00017" if i == 3 else f"cap{i}"
        np.save(root / "images" / f"{stem}.npy", R.plane(h, w, i + 1))
        n = 2 + i
        lb = np.concatenate([rng.integers(0, 7, (n, 1)).astype(np.float64), rng.uniform(0.25, 0.75, (n, 2)),
                             rng.uniform(0.1, 0.4, (n, 2))], 1)
        np.savetxt(root / "labels" / f"{stem}.txt", lb, fmt="%.6f")
    return root


@pytest.fixture(scope="module")
def planes_ref(planes_dir):
    """path -> (the definition's [3,S,S] image, labels [k,6], shapes), computed once."""
    from adaptiveisp_amd.val.loader import letterboxed_geometry, letterboxed_labels
    ref = {}
    for f in sorted(os.listdir(planes_dir / "images")):
        path = str(planes_dir / "images" / f)
        p = np.load(path)
        size, unpad, place, frame, ratio, pad, shapes = letterboxed_geometry(p.shape[0], p.shape[1], S_DATA)
        assert frame == (S_DATA, S_DATA)
        lb = letterboxed_labels(path, size, frame, ratio, pad)
        label = np.zeros((len(lb), 6), np.float32)
        label[:, 1:] = lb
        img = R.raw_load_one(p, unpad, place, S_DATA, "GRBG", "mhc", 64, 4095, gains=SENSOR["raw_gains"])
        ref[path] = (img, label, shapes)
    return ref


def _deliver(root, n_batches, **kw):
    from adaptiveisp_amd.data import ImageFolderSource
    src = ImageFolderSource(str(root / "images"), S_DATA, DEV, data_name="raw", **SENSOR, **kw)
    try:
        out = []
        for _ in range(n_batches):
            imgs, labels, paths, shapes = src.get_next_batch(2)
            out.append((torch.stack(imgs).cpu().numpy(), labels, paths, shapes))
        return out, src.serial
    finally:
        src.close()


def test_source_delivers_the_definition(planes_dir, planes_ref):
    runs = {kw: _deliver(planes_dir, 4, workers=kw[0], resize=kw[1]) for kw in ((0, "host"), (3, "host"), (3, "device"))}
    first, serial = runs[(0, "host")]
    assert serial == 8
    assert [os.path.basename(p) for b in first[:2] for p in b[2]] == ["00017.npy", "cap0.npy", "cap1.npy", "cap2.npy"]
    for imgs, labels, paths, shapes in first:                          # the pass in file order and the reshuffled wrap
        assert imgs.shape == (2, 3, S_DATA, S_DATA)
        for k, path in enumerate(paths):
            img, label, shp = planes_ref[path]
            assert _same(imgs[k], img), path
            assert np.array_equal(labels[k], label) and labels[k].dtype == np.float32 and shapes[k] == shp
    for other, _ in (runs[(3, "host")], runs[(3, "device")]):          # worker count and `resize` change nothing
        for (ia, la, pa, sa), (ib, lb, pb, sb) in zip(first, other):
            assert pa == pb and sa == sb and _same(ia, ib) and all(np.array_equal(x, y) for x, y in zip(la, lb))


# ------------------------------------------------------------------------------------------------------------ the CLI
def test_cli_val_on_raw_planes_equals_run_eval(planes_dir, tmp_path):
    from _synth import synth_state_dict
    from adaptiveisp_amd.agent import Agent
    from adaptiveisp_amd.config import cfg
    from adaptiveisp_amd.data import ImageFolderSource
    from adaptiveisp_amd.val import run_eval
    from adaptiveisp_amd.val.__main__ import _batches
    from adaptiveisp_amd.yolo import YoloEngine, yolov3
    agent = Agent(cfg, shape=(6 + len(cfg.filters), 64, 64))
    torch.save({"iter": 0, "agent_model": synth_state_dict(agent, seed=0)}, tmp_path / "agent.pth")
    cmd = ["timeout", "-k", "10", "600", sys.executable, "-m", "adaptiveisp_amd.val", "--isp-ckpt", str(tmp_path / "agent.pth"),
           "--data", str(planes_dir / "images"), "--data-name", "raw", "--cfa", "GRBG", "--raw-bits", "12", "--demosaic", "mhc",
           "--raw-gains", "1.9", "1.0", "1.6", "--img-size", str(S_DATA), "--batch-size", "2", "--project",
           str(tmp_path / "runs"), "--name", "raw"]
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    r = subprocess.run(cmd, cwd=ROOT, env=env, capture_output=True, text=True)         # a fresh child process
    assert r.returncode == 0, f"exit {r.returncode}\n{r.stdout[-3000:]}\n{r.stderr[-3000:]}"
    run = r.stdout.strip().splitlines()[-1].split("Results saved to ", 1)[1]
    res = json.load(open(os.path.join(run, "results.json")))
    assert os.path.isfile(os.path.join(run, "records.txt")) and res["seen"] == 5
    assert res["args"]["data_name"] == "raw" and res["args"]["raw_gains"] == [1.9, 1.0, 1.6]
    # the same evaluation in this process: the command line's random-init detector is seeded by --seed 0
    torch.manual_seed(0)
    det = yolov3(nc=80).to(DEV).eval()
    agent = Agent(cfg, shape=(6 + len(cfg.filters), 64, 64), device=DEV).to(DEV)
    agent.load_state_dict(synth_state_dict(agent, seed=0))
    agent.eval()
    engines = {b: YoloEngine(det, b, S_DATA, S_DATA, device=DEV) for b in (2, 1)}
    src = ImageFolderSource(str(planes_dir / "images"), S_DATA, DEV, data_name="raw", **SENSOR)
    try:
        np.random.seed(0)
        ref = run_eval(agent, lambda x: engines[x.shape[0]](x), _batches(src, len(src), 2), cfg, steps=5, nc=80,
                       records_path=str(tmp_path / "records_ref.txt"))
    finally:
        src.close()
    for k in ("mp", "mr", "map50", "map75", "map"):
        assert res[k] == ref[k], k
    assert ref["seen"] == 5 and res["instances"] == int(ref["nt"].sum())
    assert open(os.path.join(run, "records.txt")).read() == open(tmp_path / "records_ref.txt").read()
