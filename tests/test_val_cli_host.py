"""The evaluation CLI on the host (no GPU): argument handling of `python -m adaptiveisp_amd.val`, dataset YAML resolution,
the run-directory increment, the label / COCO-JSON writers against the reference's own output (tests/golden/valcli.npz),
the float -> uint8 arithmetic of the image export against the array the reference hands cv2.imwrite, and the argument
checks of the adaisp_export_u8 C entry."""
import ctypes
import json
import os
import subprocess

import numpy as np
import pytest
import torch

from adaptiveisp_amd import _lib
from adaptiveisp_amd.val import __main__ as cli
from adaptiveisp_amd.val import writers

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _text(a):
    return bytes(np.asarray(a, np.uint8)).decode("utf-8")


def export_u8_np(chw):
    """numpy restatement of adaisp_export_u8 for one [3,H,W] image: NaN -> 0, clip, * 255 in fp32, round half to even,
    RGB planes -> HWC BGR."""
    x = np.array(chw, np.float32, copy=True)
    x[np.isnan(x)] = 0
    x = np.clip(x, np.float32(0), np.float32(1)) * np.float32(255.0)
    return np.rint(x).astype(np.uint8).transpose(1, 2, 0)[:, :, ::-1]


def _base(*extra):
    return ["--isp-ckpt", "agent.pth", "--data", "images", *extra]


# ------------------------------------------------------------------------------------------------------------ arguments
@pytest.mark.parametrize("extra", [["--pipeline", "8,3,2,5"], ["--pipeline", "8,3,2,5,7", "--steps", "6"],
                                   ["--pipeline", "8,3,2,5,10"], ["--pipeline", "8,3,-1,5,7"], ["--pipeline", "8,x,2,5,7"]])
def test_pipeline_too_short_or_out_of_range_is_a_usage_error(extra, capsys):
    with pytest.raises(SystemExit) as e:
        cli.parse_args(_base(*extra))
    assert e.value.code == 2
    assert "--pipeline" in capsys.readouterr().err


def test_pipeline_parsed():
    a = cli.parse_args(_base("--pipeline", "8,3,2,5,7,1", "--steps", "5"))
    assert a.pipeline == [8, 3, 2, 5, 7, 1]
    assert cli.parse_args(_base()).pipeline is None


def test_save_param_needs_batch_one(capsys):
    with pytest.raises(SystemExit) as e:
        cli.parse_args(_base("--save-param", "--batch-size", "2"))
    assert e.value.code == 2 and "--save-param" in capsys.readouterr().err
    assert cli.parse_args(_base("--save-param")).save_param


def test_isp_ckpt_is_required():
    with pytest.raises(SystemExit):
        cli.parse_args(["--data", "images"])


@pytest.mark.parametrize("size,want", [(512, 512), (500, 512), (513, 544), (32, 32), (1, 32), (640, 640)])
def test_image_size_rounded_up_to_the_stride(size, want, capsys):
    a = cli.parse_args(_base("--img-size", str(size)))
    assert a.img_size == want
    assert ("updating to" in capsys.readouterr().out) == (size != want)


def test_lod_forces_noise_off_and_graph_yields_to_saves(capsys):
    a = cli.parse_args(_base("--add-noise", "--bri-range", "0.1", "0.3"))
    assert a.add_noise is False and a.bri_range is None
    a = cli.parse_args(_base("--data-name", "coco", "--add-noise", "--bri-range", "0.1", "0.3"))
    assert a.add_noise is True and a.bri_range == [0.1, 0.3]
    assert cli.parse_args(_base("--graph")).graph is True
    capsys.readouterr()
    for flag in ("--save-image", "--save-param"):
        assert cli.parse_args(_base("--graph", flag)).graph is False
        assert "--graph ignored" in capsys.readouterr().out


def test_increment_path(tmp_path):
    base = tmp_path / "runs" / "exp"
    assert cli.increment_path(base) == str(base)
    os.makedirs(base)
    assert cli.increment_path(base) == str(base) + "2"
    os.makedirs(str(base) + "2")
    assert cli.increment_path(base) == str(base) + "3"
    assert cli.increment_path(base, exist_ok=True) == str(base)


def _touch_images(d, names):
    from PIL import Image
    os.makedirs(d, exist_ok=True)
    for n in names:
        Image.fromarray(np.zeros((4, 4, 3), np.uint8)).save(os.path.join(d, n))


def test_yaml_resolution_dir_and_txt_list(tmp_path):
    from adaptiveisp_amd.val.loader import list_images
    root = tmp_path / "datasets" / "LOD"
    _touch_images(root / "images" / "val", ["b.png", "a.png"])
    _touch_images(root / "images" / "train", ["c.png"])
    (root / "val.txt").write_text("./images/val/b.png\n./images/val/a.png\n")
    cfgdir = tmp_path / "cfg"
    os.makedirs(cfgdir)
    y = cfgdir / "lod.yaml"
    y.write_text("path: ../datasets/LOD\ntrain: images/train\nval: val.txt\nnames:\n  0: person\n  1: bicycle\n  2: car\n")
    src, names, nc = cli.resolve_data(str(y), "val")
    assert os.path.samefile(src, root / "val.txt")
    assert names == {0: "person", 1: "bicycle", 2: "car"} and nc == 3
    assert [os.path.basename(f) for f in list_images(src)] == ["b.png", "a.png"]
    src, _, _ = cli.resolve_data(str(y), "train")
    assert os.path.samefile(src, root / "images" / "train")
    assert [os.path.basename(f) for f in list_images(src)] == ["c.png"]
    with pytest.raises(ValueError, match="test"):
        cli.resolve_data(str(y), "test")
    # an absolute `path`, `nc` next to a list of names
    y2 = cfgdir / "abs.yaml"
    y2.write_text(f"path: {root}\nval: images/val\nnc: 2\nnames: [x, y]\n")
    src, names, nc = cli.resolve_data(str(y2), "val")
    assert os.path.samefile(src, root / "images" / "val") and names == {0: "x", 1: "y"} and nc == 2
    y3 = cfgdir / "bad.yaml"
    y3.write_text(f"path: {root}\nval: images/val\nnc: 3\nnames: [x, y]\n")
    with pytest.raises(ValueError, match="nc"):
        cli.resolve_data(str(y3), "val")
    # anything that is not a YAML is the source itself
    assert cli.resolve_data(str(root / "images" / "val"), "val") == (str(root / "images" / "val"), None, None)


# ------------------------------------------------------------------------------------------------------------ writers
def _cases(g):
    return _text(g["case.names"]).split()


def test_class_map_is_the_references(golden):
    g = golden("valcli")
    assert writers.coco80_to_coco91_class() == g["class_map"].tolist()
    assert len(g["class_map"]) == 80


def test_txt_writer_reproduces_the_reference(golden, tmp_path):
    g = golden("valcli")
    assert set(_cases(g)) == {"numeric", "named", "zeros", "empty"}
    for name in _cases(g):
        predn, shape = torch.from_numpy(g[f"{name}.predn"]), tuple(int(v) for v in g[f"{name}.shape"])
        for key, conf in (("txt", False), ("txt_conf", True)):
            f = tmp_path / f"{name}_{key}.txt"
            writers.save_one_txt(predn, conf, shape, str(f))
            got = f.read_bytes() if f.exists() else b""
            assert got == _text(g[f"{name}.{key}"]).encode(), (name, key)


def test_json_writer_reproduces_the_reference(golden):
    g = golden("valcli")
    for name in _cases(g):
        jdict = []
        writers.save_one_json(torch.from_numpy(g[f"{name}.predn"]), jdict, _text(g[f"{name}.path"]),
                              writers.coco80_to_coco91_class())
        want = json.loads(_text(g[f"{name}.json"]))
        assert jdict == want, name
        assert json.dumps(jdict) == _text(g[f"{name}.json"]), name
    assert writers.image_id("/x/000000397133.jpg") == 397133 and writers.image_id("/x/night_street-1.png") == "night_street-1"


def test_export_arithmetic_matches_what_the_reference_hands_cv2(golden):
    """OpenCV's float -> 8U conversion of the array save_img passes to cv2.imwrite (round half to even, saturate) is the
    numpy restatement of adaisp_export_u8 — including NaN, +-inf, negatives, values > 1 and exact .5 products."""
    g = golden("valcli")
    assert len(g["ties"]) == 255 and np.all(np.float32(g["ties"]) * np.float32(255.0) % 1 == 0.5)
    k = 0
    while f"img{k}" in g.files:
        saved = g[f"saved{k}"]
        assert saved.dtype == np.float32
        cv2_bytes = np.clip(np.rint(saved), 0, 255).astype(np.uint8)
        np.testing.assert_array_equal(export_u8_np(g[f"img{k}"]), cv2_bytes)
        k += 1
    assert k == 3


def test_image_writer_round_trips_lossless_formats(tmp_path):
    rng = np.random.default_rng(0)
    bgr = rng.integers(0, 256, (7, 13, 3), dtype=np.uint8)
    w = writers.ImageWriter(workers=2, depth=2)
    for ext in ("png", "bmp", "tif", "tiff", "jpg"):
        w.submit(str(tmp_path / f"a.{ext}"), bgr)
    w.close()
    from adaptiveisp_amd.val.loader import imread_bgr
    for ext in ("png", "bmp", "tif", "tiff"):
        np.testing.assert_array_equal(imread_bgr(str(tmp_path / f"a.{ext}")), bgr)
    assert imread_bgr(str(tmp_path / "a.jpg")).shape == bgr.shape


def test_image_writer_close_raises_a_failed_write_unless_told_not_to(tmp_path):
    bgr = np.zeros((2, 2, 3), np.uint8)
    w = writers.ImageWriter(workers=1)
    w.submit(str(tmp_path / "missing_dir" / "a.png"), bgr)
    w.submit(str(tmp_path / "b.png"), bgr)
    with pytest.raises(OSError):
        w.close()
    w = writers.ImageWriter(workers=1)
    w.submit(str(tmp_path / "missing_dir" / "c.png"), bgr)
    w.submit(str(tmp_path / "d.png"), bgr)
    w.close(raise_errors=False)                       # a caller unwinding from its own error: waits, raises nothing
    assert (tmp_path / "b.png").exists() and (tmp_path / "d.png").exists()
    w.close()                                         # closed: a second close is a no-op


class _FakeSource:
    """ImageFolderSource's get_next_batch contract on the host: labels [k,6] with column 0 zero, classes 0..6."""

    def get_next_batch(self, n):
        imgs = [torch.zeros(3, 4, 4) for _ in range(n)]
        labels = [np.array([[0, 3, 0.5, 0.5, 0.1, 0.1], [0, 6, 0.2, 0.3, 0.1, 0.2]], np.float32) for _ in range(n)]
        return imgs, labels, [f"{i}.png" for i in range(n)], [((4, 4), ((1.0, 1.0), (0.0, 0.0)))] * n


@pytest.mark.parametrize("single_cls", [False, True])
def test_batches_ragged_and_single_cls_merges_label_classes(single_cls):
    out = list(cli._batches(_FakeSource(), 5, 2, single_cls))
    assert [b[0].shape[0] for b in out] == [2, 2, 1]
    for im, t, paths, shapes in out:
        assert t[:, 0].tolist() == [k for k in range(im.shape[0]) for _ in range(2)]
        assert t[:, 1].tolist() == ([0.0] * len(t) if single_cls else [3.0, 6.0] * im.shape[0])


# ------------------------------------------------------------------------------------------------------------ C entry
def test_cabi_export_rejects_bad_arguments():
    L = _lib.load()
    p = ctypes.c_void_p(4096)                         # never dereferenced: every call below fails its checks first
    E = -1
    assert L.adaisp_export_u8(None, p, 1, 2, 2, None) == E
    assert L.adaisp_export_u8(p, None, 1, 2, 2, None) == E
    for B, H, W in ((0, 2, 2), (-1, 2, 2), (1, 0, 2), (1, 2, 0), (1, -5, 2), (1, 2, -5)):
        assert L.adaisp_export_u8(p, p, B, H, W, None) == E, (B, H, W)
    assert L.adaisp_export_u8(p, p, 65536, 2, 2, None) == -4
    assert "adaisp_export_u8" in _lib.EXPORTS and _lib.ABI_VERSION == 9


def test_export_wrapper_rejects_host_tensors():
    with pytest.raises(_lib.AdaispError, match="device"):
        _lib.export_u8(torch.zeros(1, 3, 2, 2))


# ------------------------------------------------------------------------------------------------------------ fixture
def test_regen_check_valcli_reproduces_the_fixture():
    """tools/regen_check.sh valcli: the generator, run against the reference, rewrites valcli.npz with 0 differences
    (where the reference checkout is present: the build container)."""
    import inspect
    import sys
    sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
    import gen_valcli
    ref = inspect.signature(gen_valcli.import_reference_val).parameters["root"].default
    if not os.path.isdir(ref):
        pytest.skip("the reference checkout is not on this machine")
    r = subprocess.run(["bash", os.path.join(ROOT, "tools", "regen_check.sh"), "valcli"], cwd=ROOT, capture_output=True,
                       text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "valcli.npz: 33 arrays, 0 differing" in r.stdout and "0 differences" in r.stdout
