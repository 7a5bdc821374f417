"""The evaluation CLI on the MI355X: the adaisp_export_u8 kernel bit-exact against the reference's save_img arithmetic
(tests/golden/valcli.npz) and its numpy restatement, and `python -m adaptiveisp_amd.val` end to end in a subprocess
against an in-process run_eval on LODImages."""
import json
import os
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest
import torch


pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")


def export_u8_np(chw):
    """numpy restatement of adaisp_export_u8 for one [3,H,W] image (as tests/test_val_cli_host.py)."""
    x = np.array(chw, np.float32, copy=True)
    x[np.isnan(x)] = 0
    x = np.clip(x, np.float32(0), np.float32(1)) * np.float32(255.0)
    return np.rint(x).astype(np.uint8).transpose(1, 2, 0)[:, :, ::-1]


def _ref(x):
    return np.stack([export_u8_np(im) for im in x])


def _images(B, H, W, seed, ties):
    rng = np.random.default_rng(seed)
    x = rng.uniform(-0.25, 1.25, (B, 3, H, W)).astype(np.float32)
    flat = x.reshape(-1)
    special = np.array([np.nan, np.inf, -np.inf, -0.0, 2.0, -3.0, 1.0, 0.0], np.float32)
    k = min(flat.size, 64)
    idx = rng.choice(flat.size, size=k, replace=False)
    pool = np.concatenate([special, ties])
    flat[idx] = pool[rng.integers(0, pool.size, k)]
    return x


def test_export_matches_the_reference_arrays(golden):
    from adaptiveisp_amd import _lib
    g = golden("valcli")
    k = 0
    while f"img{k}" in g.files:
        want = np.clip(np.rint(g[f"saved{k}"]), 0, 255).astype(np.uint8)     # cv2.imwrite's float -> 8U
        got = _lib.export_u8(torch.from_numpy(g[f"img{k}"][None].copy()).to(DEV)).cpu().numpy()[0]
        np.testing.assert_array_equal(got, want)
        k += 1
    ties = torch.from_numpy(g["ties"].copy()).reshape(1, 1, 1, -1).expand(1, 3, 1, -1).contiguous()
    got = _lib.export_u8(ties.to(DEV)).cpu().numpy()
    assert (got.astype(np.int64) % 2 == 0).all()                                  # every tie went to the even neighbour


@pytest.mark.parametrize("B", [1, 3, 8])
@pytest.mark.parametrize("H,W", [(1, 1), (3, 5), (7, 129), (512, 512), (720, 1280)])
def test_export_bit_exact(golden, B, H, W):
    from adaptiveisp_amd import _lib
    x = _images(B, H, W, 100 * B + H, golden("valcli")["ties"])
    got = _lib.export_u8(torch.from_numpy(x).to(DEV)).cpu().numpy()
    assert got.shape == (B, H, W, 3) and got.dtype == np.uint8
    np.testing.assert_array_equal(got, _ref(x))


@pytest.mark.parametrize("in_off", [0, 1, 2, 4])
@pytest.mark.parametrize("out_off", [0, 1, 3, 4, 16])
@pytest.mark.parametrize("H,W", [(8, 16), (7, 129)])
def test_export_any_alignment_and_nothing_past_the_output(golden, in_off, out_off, H, W):
    """Input views at 4-byte offsets (the scalar path) and 16-byte ones (the vector path), outputs at any byte offset;
    sentinel bytes before and after the output are untouched."""
    from adaptiveisp_amd import _lib
    B = 3
    x = _images(B, H, W, 7 + in_off, golden("valcli")["ties"])
    n = x.size
    buf = torch.full((n + in_off + 8,), 0.5, dtype=torch.float32, device=DEV)
    view = buf[in_off:in_off + n].view(B, 3, H, W)
    view.copy_(torch.from_numpy(x))
    nbytes = B * H * W * 3
    obuf = torch.full((out_off + nbytes + 64,), 0xA5, dtype=torch.uint8, device=DEV)
    out = obuf[out_off:out_off + nbytes].view(B, H, W, 3)
    _lib.export_u8(view, out=out)
    host = obuf.cpu().numpy()
    np.testing.assert_array_equal(host[out_off:out_off + nbytes].reshape(B, H, W, 3), _ref(x))
    assert (host[:out_off] == 0xA5).all() and (host[out_off + nbytes:] == 0xA5).all()


# ------------------------------------------------------------------------------------------------------------ the CLI
def _write_dataset(root):
    """Five PNGs of different native sizes (one with a numeric stem) + YOLO labels of the fixture detector's 7 classes."""
    from PIL import Image
    os.makedirs(root / "images"); os.makedirs(root / "labels")
    rng = np.random.default_rng(21)
    for i, (h, w) in enumerate([(300, 400), (256, 192), (333, 250), (180, 320), (240, 240)]):
        base = rng.random((h // 8 + 1, w // 8 + 1, 3))
        im = np.kron(base, np.ones((8, 8, 1)))[:h, :w] * 0.4 + rng.random((h, w, 3)) * 0.1
        stem = "00017" if i == 3 else f"img{i}"
        Image.fromarray((im * 255).astype(np.uint8)).save(root / "images" / f"{stem}.png")
        n = 2 + i
        lb = np.concatenate([rng.integers(0, 7, (n, 1)).astype(np.float64), rng.uniform(0.25, 0.75, (n, 2)),
                             rng.uniform(0.1, 0.4, (n, 2))], 1)
        np.savetxt(root / "labels" / f"{stem}.txt", lb, fmt="%.6f")


def _agent_ckpt(path):
    from _synth import synth_state_dict
    from adaptiveisp_amd.agent import Agent
    from adaptiveisp_amd.config import cfg
    agent = Agent(cfg, shape=(6 + len(cfg.filters), 64, 64))
    torch.save({"iter": 0, "agent_model": synth_state_dict(agent, seed=0)}, path)


S = 256


def _cli(tmp, name, *extra):
    cmd = ["timeout", "-k", "10", "600", sys.executable, "-m", "adaptiveisp_amd.val", "--isp-ckpt", str(tmp / "agent.pth"),
           "--detector-ckpt", os.path.join(GOLD, "yolov3_w0625_refpickle.pt"), "--data", str(tmp / "data" / "images"),
           "--img-size", str(S), "--batch-size", "2", "--project", str(tmp / "runs"), "--name", name, *extra]
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    r = subprocess.run(cmd, cwd=ROOT, env=env, capture_output=True, text=True)
    assert r.returncode == 0, f"exit {r.returncode}\n{r.stdout[-3000:]}\n{r.stderr[-3000:]}"
    run = Path(r.stdout.strip().splitlines()[-1].split("Results saved to ", 1)[1])
    res = json.load(open(run / "results.json"))
    return run, res, r.stdout


def _metrics(res):
    return {k: v for k, v in res.items() if k not in ("ms_per_image", "args", "save_dir")}


@pytest.fixture(scope="module")
def cli_run(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("valcli")
    _write_dataset(tmp / "data")
    _agent_ckpt(tmp / "agent.pth")
    run, res, out = _cli(tmp, "exp", "--save-image", "--save-txt", "--save-conf", "--save-json")
    return tmp, run, res, out


def test_cli_end_to_end_equals_run_eval(cli_run):
    from _synth import synth_state_dict
    from adaptiveisp_amd.agent import Agent
    from adaptiveisp_amd.config import cfg
    from adaptiveisp_amd import _lib
    from adaptiveisp_amd.val import run_eval, scale_boxes, writers
    from adaptiveisp_amd.val.loader import LODImages, imread_bgr
    from adaptiveisp_amd.yolo import YoloEngine
    from adaptiveisp_amd.yolo.checkpoint import load_detector_checkpoint
    tmp, run, res, out = cli_run
    assert "mAP50-95" in out and "Results saved to" in out
    det = load_detector_checkpoint(os.path.join(GOLD, "yolov3_w0625_refpickle.pt")).to(DEV).eval()
    agent = Agent(cfg, shape=(6 + len(cfg.filters), 64, 64), device=DEV).to(DEV)
    agent.load_state_dict(synth_state_dict(agent, seed=0))
    agent.eval()
    engines = {b: YoloEngine(det, b, S, S, device=DEV) for b in (2, 1)}
    batches = list(LODImages(str(tmp / "data" / "images"), img_size=S, batch_size=2))
    assert [b[0].shape[0] for b in batches] == [2, 2, 1]
    shapes = {p: s for b in batches for p, s in zip(b[2], b[3])}
    np.random.seed(0)
    details = []
    ref = run_eval(agent, lambda x: engines[x.shape[0]](x), batches, cfg, steps=5, nc=det.model[-1].nc,
                   records_path=str(tmp / "records_ref.txt"), details=details)
    # metrics and records
    for k in ("mp", "mr", "map50", "map75", "map"):
        assert res[k] == ref[k], k
    assert res["seen"] == ref["seen"] == 5 and res["instances"] == int(ref["nt"].sum())
    assert [r["name"] for r in res["classes"]] == [str(det.names[int(c)]) for c in ref["ap_class"]]
    assert [r["p"] for r in res["classes"]] == [float(v) for v in ref["p"]]
    assert open(run / "records.txt").read() == open(tmp / "records_ref.txt").read()
    # labels and COCO JSON: the host writers on run_eval's detections, mapped to native space where run_eval does it
    jdict, want_txt = [], {}
    for d in details:
        if d["pred"].shape[0] == 0:
            continue
        predn = d["pred"].to(DEV).clone()
        shape = shapes[d["path"]]
        scale_boxes((S, S), predn[:, :4], shape[0], shape[1])
        predn = predn.cpu()
        want_txt[os.path.splitext(os.path.basename(d["path"]))[0] + ".txt"] = "".join(writers.txt_rows(predn, True, shape[0]))
        writers.save_one_json(predn, jdict, d["path"], writers.coco80_to_coco91_class())
    assert sorted(os.listdir(run / "labels")) == sorted(want_txt)
    for f, text in want_txt.items():
        assert open(run / "labels" / f).read() == text, f
    got_json = json.load(open(run / "yolov3_w0625_refpickle_predictions.json"))
    assert got_json == json.loads(json.dumps(jdict)) and any(isinstance(r["image_id"], int) for r in got_json)
    # step images: every step that ran, the last one decoding to the export of the final retouched image
    steps_run = {name: sum(v != "-1" for v in row) for name, row in ref["records"]}
    n_files = sum(len(fs) for _, _, fs in os.walk(run / "img_results"))
    assert n_files == sum(steps_run.values()) == 5 * 5
    for d in details:
        name = os.path.basename(d["path"])
        png = imread_bgr(str(run / "img_results" / f"step-{steps_run[name] - 1}" / name))
        np.testing.assert_array_equal(png, _lib.export_u8(d["retouch"][None].to(DEV)).cpu().numpy()[0])


def test_cli_graph_equals_eager(cli_run):
    tmp, run, res, _ = cli_run
    grun, gres, out = _cli(tmp, "exp", "--graph")
    assert grun == tmp / "runs" / "exp2" and run == tmp / "runs" / "exp"                     # incremented
    assert gres["args"]["graph"] is True
    assert _metrics(gres) == _metrics(res)
    assert open(grun / "records.txt").read() == open(run / "records.txt").read()


def test_cli_pipeline_in_records(cli_run):
    tmp = cli_run[0]
    run, res, _ = _cli(tmp, "pipe", "--pipeline", "8,3,2,5,7")
    rows = open(run / "records.txt").read().strip().splitlines()
    assert len(rows) == 6
    assert all(r.split(",", 1)[1] == "8,3,2,5,7" for r in rows[1:])


def test_cli_coco_noise_is_seeded(cli_run):
    tmp = cli_run[0]
    outs = []
    for name in ("coco_a", "coco_b"):
        run, res, _ = _cli(tmp, name, "--data-name", "coco", "--add-noise", "--seed", "3", "--save-txt", "--save-conf")
        labels = {f: open(run / "labels" / f).read() for f in sorted(os.listdir(run / "labels"))}
        outs.append((_metrics(res), open(run / "records.txt").read(), labels))
    assert outs[0] == outs[1] and outs[0][0]["seen"] == 5


def _models():
    from _synth import synth_state_dict
    from adaptiveisp_amd.agent import Agent
    from adaptiveisp_amd.config import cfg
    from adaptiveisp_amd.yolo import YoloEngine
    from adaptiveisp_amd.yolo.checkpoint import load_detector_checkpoint
    det = load_detector_checkpoint(os.path.join(GOLD, "yolov3_w0625_refpickle.pt")).to(DEV).eval()
    agent = Agent(cfg, shape=(6 + len(cfg.filters), 64, 64), device=DEV).to(DEV)
    agent.load_state_dict(synth_state_dict(agent, seed=0))
    agent.eval()
    engines = {b: YoloEngine(det, b, S, S, device=DEV) for b in (2, 1)}
    return cfg, agent, det, lambda x: engines[x.shape[0]](x)


def test_cli_single_cls_merges_the_labels(cli_run):
    """--single-cls: every label counts as class 0 (the reference's dataset merges them), so a detection of any class can
    match any label — the result equals run_eval on labels merged to class 0, with one class."""
    from adaptiveisp_amd.val import run_eval
    from adaptiveisp_amd.val.loader import LODImages
    tmp, _, res_multi, _ = cli_run
    run, res, _ = _cli(tmp, "single", "--single-cls")
    cfg, agent, _, detector = _models()
    batches, classes = [], set()
    for im, t, paths, shapes in LODImages(str(tmp / "data" / "images"), img_size=S, batch_size=2):
        t = t.clone()
        classes |= set(t[:, 1].int().tolist())
        t[:, 1] = 0
        batches.append((im, t, paths, shapes))
    assert len(classes) > 1                                      # the fixture's labels span several classes
    np.random.seed(0)
    ref = run_eval(agent, detector, batches, cfg, steps=5, nc=1, single_cls=True)
    for k in ("mp", "mr", "map50", "map75", "map"):
        assert res[k] == ref[k], k
    assert res["instances"] == res_multi["instances"] == int(ref["nt"].sum()) and len(ref["nt"]) == 1
    assert [r["name"] for r in res["classes"]] == ["c0"] and res["classes"][0]["instances"] == res["instances"]


def test_early_exit_writes_only_the_steps_that_ran(cli_run, tmp_path):
    """steps = 7 > cfg.test_steps: `stopped` is raised by the fifth step and the loop exits; only steps 0..4 are written
    (the reference indexes past its step list there). run_eval creates the step directories itself; the CLI also
    creates all 7 up front, as the reference does, and leaves 5 and 6 empty."""
    from adaptiveisp_amd.val import run_eval
    from adaptiveisp_amd.val.loader import LODImages
    tmp = cli_run[0]
    cfg, agent, _, detector = _models()
    assert cfg.test_steps == 5
    batches = list(LODImages(str(tmp / "data" / "images"), img_size=S, batch_size=2))
    names = sorted(os.path.basename(p) for b in batches for p in b[2])
    np.random.seed(0)
    out = tmp_path / "imgs"                                     # does not exist yet
    res = run_eval(agent, detector, batches, cfg, steps=7, image_dir=str(out))
    assert all(row[5:] == ["-1", "-1"] and "-1" not in row[:5] for _, row in res["records"])
    assert sorted(os.listdir(out)) == [f"step-{i}" for i in range(5)]
    for i in range(5):
        assert sorted(os.listdir(out / f"step-{i}")) == names
    run, cres, _ = _cli(tmp, "early", "--steps", "7", "--save-image")
    rows = open(run / "records.txt").read().strip().splitlines()[1:]
    assert len(rows) == 5 and all(r.endswith(",-1,-1") for r in rows)
    for i in range(7):
        assert sorted(os.listdir(run / "img_results" / f"step-{i}")) == (names if i < 5 else [])
