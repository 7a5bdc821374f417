"""adaisp_resize_u8 on the MI355X (csrc/isp_resize.hip) and ImageFolderSource(resize="device"): the kernel bit for bit
against the numpy restatement (tests/_resizeref.py) in all four modes at odd byte offsets, against the host kernels of
val/loader.py, under hipGraph capture; the device-resize source against the host-resize source on a photo-sized toy
dataset; and both command lines end to end with --resize device."""
import json
import os
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

from _resizeref import photo, resize_ref
from adaptiveisp_amd import _lib
from adaptiveisp_amd.data import ImageFolderSource
from adaptiveisp_amd.resize import TapPlan, choose_mode
from adaptiveisp_amd.val.loader import resize_area_u8, resize_linear_u8

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
FILL = 0xA5


def _stage(jobs, gap=0, dst_gap=0):
    """jobs: (img, (h, w), area). Packs the sources with `gap` filler bytes before each (odd: odd offsets) and the
    destinations likewise; returns (src, dst, desc, tabs, records, [(dst offset, (h, w))])."""
    plan = TapPlan()
    chunks, off, doff, outs = [], gap, dst_gap, []
    for im, (h, w), area in jobs:
        chunks += [np.full(gap, 77, np.uint8), im.reshape(-1)]
        plan.add(im.shape[:2], (h, w), area, off, doff)
        outs.append((doff, (h, w)))
        off += gap + im.size
        doff += dst_gap + h * w * 3
    src = torch.from_numpy(np.concatenate(chunks + [np.full(gap, 77, np.uint8)])).to(DEV)
    dst = torch.full((doff + 64,), FILL, dtype=torch.uint8, device=DEV)
    rec = plan.descriptors()
    desc = torch.from_numpy(rec.view(np.uint8).copy()).to(DEV)
    tab = plan.table()
    tabs = torch.from_numpy(tab.copy()).to(DEV) if tab.size else None
    return src, dst, desc, tabs, rec, outs


def _run(jobs, gap=0, dst_gap=0):
    src, dst, desc, tabs, rec, outs = _stage(jobs, gap, dst_gap)
    _lib.resize_u8(src, dst, desc, tabs, rec)
    torch.cuda.synchronize()
    host = dst.cpu().numpy()
    got = [host[o:o + h * w * 3].reshape(h, w, 3) for o, (h, w) in outs]
    written = np.zeros(host.size, bool)
    for o, (h, w) in outs:
        written[o:o + h * w * 3] = True
    assert (host[~written] == FILL).all()                                     # nothing outside the destinations
    return got, rec


def test_mixed_mode_batch_at_odd_offsets():
    jobs = [(photo(480, 640, 1), (384, 512), True),          # AREA
            (photo(768, 1024, 2), (384, 512), True),         # AREA_INT 2 x 2
            (photo(90, 120, 3), (30, 40), True),             # AREA_INT 3 x 3
            (photo(300, 400, 4), (384, 512), True),          # LINEAR (enlarge)
            (photo(341, 512, 5), (340, 512), False),         # LINEAR (letterbox's overshoot)
            (photo(57, 33, 6), (57, 33), True),              # COPY
            (photo(1, 300, 7), (1, 97), True),               # 1 x N, AREA
            (photo(300, 1, 8), (97, 1), True)]               # N x 1, AREA
    assert sorted({choose_mode(im.shape[:2], hw, a) for im, hw, a in jobs}) == [0, 1, 2, 3]
    for gap, dst_gap in ((0, 0), (3, 1), (7, 5)):
        got, rec = _run(jobs, gap, dst_gap)
        for k, (im, hw, area) in enumerate(jobs):
            assert np.array_equal(got[k], resize_ref(im, hw, area)), (k, rec[k]["mode"], gap)


def test_one_pixel_images():
    jobs = [(photo(1, 1, 1), (3, 5), True), (photo(3, 1, 2), (1, 1), True), (photo(1, 9, 3), (1, 4), True),
            (photo(9, 1, 4), (4, 1), True), (photo(1, 7, 5), (1, 7), True), (photo(2, 1024, 6), (1, 512), True),
            (photo(1, 5, 7), (4, 9), False), (photo(6, 1, 8), (2, 1), False)]
    got, _ = _run(jobs, gap=1, dst_gap=3)
    for k, (im, hw, area) in enumerate(jobs):
        assert np.array_equal(got[k], resize_ref(im, hw, area)), k


def test_large_source_to_an_odd_destination_offset():
    im = photo(3024, 4032, 11)
    got, rec = _run([(im, (384, 512), True)], gap=5, dst_gap=13)
    assert rec[0]["mode"] == _lib.RESIZE_AREA
    assert np.array_equal(got[0], resize_ref(im, (384, 512), True))


SWEEP = [((480, 640), (384, 512)), ((384, 512), (480, 640)), ((333, 500), (341, 512)), ((7, 5), (3, 2)),
         ((100, 147), (436, 641)), ((436, 641), (436, 640)), ((768, 1024), (384, 512)), ((1152, 1536), (384, 512)),
         ((64, 64), (16, 32)), ((1024, 2), (512, 1)), ((427, 640), (342, 512)), ((720, 1280), (288, 512))]


def test_bit_exact_to_the_host_kernels():
    """resize_linear_u8 and resize_area_u8 themselves (the general area branch included: these sizes are equal to the
    restatement on every sample, tests/test_resize_host.py)."""
    ims = [photo(*s, seed=i) for i, (s, _) in enumerate(SWEEP)]
    for area, host in ((False, resize_linear_u8), (True, resize_area_u8)):
        got, _ = _run([(im, d, area) for im, (_, d) in zip(ims, SWEEP)], gap=3, dst_gap=1)
        for k, (im, (_, d)) in enumerate(zip(ims, SWEEP)):
            assert np.array_equal(got[k], host(im, (d[1], d[0]))), (k, area)


def test_graph_replay_matches_eager():
    jobs = [(photo(480, 640, 1), (384, 512), True), (photo(300, 400, 2), (384, 512), True),
            (photo(768, 1024, 3), (384, 512), True), (photo(341, 512, 4), (340, 512), False)]
    src, dst, desc, tabs, rec, _ = _stage(jobs, gap=3, dst_gap=1)
    _lib.resize_u8(src, dst, desc, tabs, rec)
    torch.cuda.synchronize()
    eager = dst.clone()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        _lib.resize_u8(src, dst, desc, tabs, rec)
    torch.cuda.current_stream().wait_stream(s)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        _lib.resize_u8(src, dst, desc, tabs, rec)
    dst.fill_(FILL)                               # what the replay does not write again stays different from eager
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(dst, eager)


# ------------------------------------------------------------------------------------------- the replay source
PHOTO_SIZES = [(480, 640), (640, 480), (375, 500), (427, 640), (512, 512), (720, 1280), (333, 500), (640, 427)]
EXTRA = [(700, 1050), (100, 147)]                  # ceil overshoots at S = 640 (after a shrink, after an enlargement)


def _write_dataset(root, sizes, seed=0):
    from PIL import Image
    rs = np.random.RandomState(seed)
    os.makedirs(root / "images")
    os.makedirs(root / "labels")
    for i, (h, w) in enumerate(sizes):
        Image.fromarray(photo(h, w, 100 + i)).save(root / "images" / f"{i:03d}.png")
        if i % 4:
            n = 1 + i % 3
            lb = np.concatenate([rs.randint(0, 7, (n, 1)), rs.uniform(0.25, 0.75, (n, 2)), rs.uniform(0.1, 0.4, (n, 2))], 1)
            np.savetxt(root / "labels" / f"{i:03d}.txt", lb, fmt="%.6f")


@pytest.fixture(scope="module")
def photo_data(tmp_path_factory):
    root = tmp_path_factory.mktemp("photos")
    _write_dataset(root, PHOTO_SIZES + EXTRA)
    return root


def _batches(root, S, resize, workers=4, data_name="lod", noise=False, seed=0, sizes=(4, 4, 2)):
    src = ImageFolderSource(str(root / "images"), S, DEV, data_name=data_name, add_noise=noise, seed=seed,
                            workers=workers, resize=resize)
    try:
        out = []
        for n in sizes:
            imgs, labels, paths, shapes = src.get_next_batch(n)
            out.append((torch.stack(imgs).cpu(), [lb.copy() for lb in labels], list(paths), list(shapes)))
        return out, src.serial
    finally:
        src.close()


@pytest.mark.parametrize("S", [512, 640])
def test_source_device_resize_equals_host_resize(photo_data, S):
    host, ns_h = _batches(photo_data, S, "host")
    dev, ns_d = _batches(photo_data, S, "device")
    assert ns_h == ns_d
    for (hi, hl, hp, hs), (di, dl, dp, ds) in zip(host, dev):
        assert torch.equal(hi, di)
        assert hp == dp and hs == ds
        assert len(hl) == len(dl) and all(np.array_equal(a, b) for a, b in zip(hl, dl))


def test_source_device_resize_coco_noise_and_workers(photo_data):
    S = 640
    host, _ = _batches(photo_data, S, "host", data_name="coco", noise=True, seed=3)
    dev, _ = _batches(photo_data, S, "device", data_name="coco", noise=True, seed=3)
    dev0, _ = _batches(photo_data, S, "device", workers=0, data_name="coco", noise=True, seed=3)
    for a, b, c in zip(host, dev, dev0):
        assert torch.equal(a[0], b[0]) and torch.equal(b[0], c[0])
        assert a[2] == b[2] == c[2] and a[3] == b[3] == c[3]


# ------------------------------------------------------------------------------------------- command lines
def test_cli_trains_with_device_resize(photo_data):
    cache = os.path.join(ROOT, "adaptiveisp_amd", "yolo", "tuning", "mi355x.json")
    saved = open(cache, "rb").read()              # the CLI autotunes into the committed table: give it back as it was
    try:
        r = subprocess.run(["timeout", "-k", "10", "600", sys.executable, "-m", "adaptiveisp_amd.train", "--data",
                            str(photo_data / "images"), "--data-name", "coco", "--add-noise", "--resize", "device",
                            "--batch", "2", "--size", "128", "--iters", "30", "--data-workers", "2"],
                           cwd=ROOT, capture_output=True, text=True)
    finally:
        with open(cache, "wb") as f:
            f.write(saved)
    assert r.returncode == 0, r.stderr[-3000:]
    line = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1])
    assert line["data"] == f"coco (unprocess, noise): {len(PHOTO_SIZES + EXTRA)} files, device resize", line["data"]
    assert line["ms_per_iter"] > 0


def _val(tmp, data, name, resize):
    from test_gpu_val_cli import _agent_ckpt
    if not (tmp / "agent.pth").exists():
        _agent_ckpt(tmp / "agent.pth")
    cmd = ["timeout", "-k", "10", "600", sys.executable, "-m", "adaptiveisp_amd.val", "--isp-ckpt", str(tmp / "agent.pth"),
           "--detector-ckpt", os.path.join(GOLD, "yolov3_w0625_refpickle.pt"), "--data", str(data / "images"),
           "--img-size", "320", "--batch-size", "3", "--project", str(tmp / "runs"), "--name", name, "--resize", resize,
           "--save-txt", "--save-conf"]
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    r = subprocess.run(cmd, cwd=ROOT, env=env, capture_output=True, text=True)
    assert r.returncode == 0, f"exit {r.returncode}\n{r.stdout[-3000:]}\n{r.stderr[-3000:]}"
    run = Path(r.stdout.strip().splitlines()[-1].split("Results saved to ", 1)[1])
    res = json.load(open(run / "results.json"))
    labels = {f: open(run / "labels" / f).read() for f in sorted(os.listdir(run / "labels"))}
    return {k: v for k, v in res.items() if k not in ("ms_per_image", "args", "save_dir")}, \
        open(run / "records.txt").read(), labels, res["args"]


def test_cli_val_device_resize_equals_host(photo_data, tmp_path):
    host = _val(tmp_path, photo_data, "host", "host")
    dev = _val(tmp_path, photo_data, "dev", "device")
    assert host[3]["resize"] == "host" and dev[3]["resize"] == "device"
    assert dev[:3] == host[:3] and host[0]["seen"] == len(PHOTO_SIZES + EXTRA)
