"""ImageFolderSource(data_name="raw") with a sensor calibration and per-capture sidecars on the MI355X: every batch is
adaisp_raw_load of adaisp_raw_correct of the plane, bit for bit the two numpy definitions composed
(_rawref.raw_load_one(_rawfixref.correct(plane, ...), ...)); without the options nothing changes; the evaluation command
line takes --raw-cal / --raw-meta."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import _rawfixref as X
import _rawref as R
from adaptiveisp_amd.rawcal import RawCalibration, read_sidecar, resolve

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
S = 64
CFA, RUN_BLACK, RUN_WHITE, RAW_GAINS = "GRBG", 64, 4095, (1.9, 1.0, 1.6)
SIDECARS = {"cap0": {"black_level": [250, 256, 258, 262], "white_level": 16383, "gains": [2.1, 1.0, 1.4]},
            "cap1": {"black_level": 70},
            "cap2": {"gains": [1.5, 1.0, 2.0], "iso": 3200}}              # cap3: none


def _same(got, want):
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want, dtype=np.float32)
    return got.shape == want.shape and np.array_equal(got.view(np.uint32), want.view(np.uint32))


@pytest.fixture(scope="module")
def folder(tmp_path_factory):
    """Four planes of different native sizes (shrunk, kept and enlarged at 64), three with sidecars, and a calibration."""
    root = tmp_path_factory.mktemp("rawfix")
    os.makedirs(root / "images")
    for i, (h, w) in enumerate([(90, 130), (64, 48), (37, 53), (50, 64)]):
        white = 16383 if i == 0 else 4000
        np.save(root / "images" / f"cap{i}.npy", X.plane(h, w, i + 1, black=256 if i == 0 else 64, white=white, hot=0.01))
        if f"cap{i}" in SIDECARS:
            json.dump(SIDECARS[f"cap{i}"], open(root / "images" / f"cap{i}.json", "w"))
    RawCalibration((60.0, 64.0, 66.5, 71.0), 4000, X.table(5, 7, 9), 40, CFA).save(root / "cal.npz")
    return root


def _source(folder, demosaic, **kw):
    from adaptiveisp_amd.data import ImageFolderSource
    return ImageFolderSource(str(folder / "images"), S, DEV, data_name="raw", cfa=CFA, raw_bits=12, demosaic=demosaic,
                             raw_gains=RAW_GAINS, workers=0, **kw)


def _batches(src, n=2, size=2):
    try:
        out = []
        for _ in range(n):
            imgs, _labels, paths, _shapes = src.get_next_batch(size)
            out.append((torch.stack(imgs).cpu().numpy(), paths))
        return out
    finally:
        src.close()


def _want(path, cal, meta_on, demosaic):
    from adaptiveisp_amd.val.loader import letterboxed_geometry
    p = np.load(path)
    meta = (read_sidecar(path) or {}) if meta_on else {}
    black, white = resolve(cal, meta, RUN_BLACK, RUN_WHITE)
    fixed = X.correct(p, black, X.scales(black, white, RUN_BLACK, RUN_WHITE), RUN_BLACK, None if cal is None else cal.dpc,
                      None if cal is None else cal.shading)
    _size, unpad, place, *_rest = letterboxed_geometry(p.shape[0], p.shape[1], S)
    return R.raw_load_one(fixed, unpad, place, S, CFA, demosaic, RUN_BLACK, RUN_WHITE, gains=meta.get("gains", RAW_GAINS))


@pytest.mark.parametrize("demosaic", ("bilinear", "mhc"))
def test_source_delivers_the_two_definitions_composed(folder, demosaic):
    cal = RawCalibration.load(folder / "cal.npz")
    seen = 0
    for imgs, paths in _batches(_source(folder, demosaic, raw_calibration=cal, raw_meta=True)):
        for k, path in enumerate(paths):
            assert _same(imgs[k], _want(path, cal, True, demosaic)), path
            seen += 1
    assert seen == 4
    for imgs, paths in _batches(_source(folder, demosaic, raw_meta=True)):               # sidecars alone
        for k, path in enumerate(paths):
            assert _same(imgs[k], _want(path, None, True, demosaic)), path
    for imgs, paths in _batches(_source(folder, demosaic, raw_calibration=str(folder / "cal.npz"))):   # the file alone
        for k, path in enumerate(paths):
            assert _same(imgs[k], _want(path, cal, False, demosaic)), path
    a = _want(str(folder / "images" / "cap0.npy"), cal, True, demosaic)
    assert not _same(a, _want(str(folder / "images" / "cap0.npy"), None, False, demosaic))


@pytest.mark.parametrize("demosaic", ("bilinear", "mhc"))
def test_identity_calibration_and_none_agree(folder, demosaic):
    plain = _batches(_source(folder, demosaic))
    src = _source(folder, demosaic, raw_calibration=RawCalibration(RUN_BLACK, RUN_WHITE, cfa=CFA))
    assert src._rawfix
    same = _batches(src)
    for (ia, pa), (ib, pb) in zip(plain, same):
        assert pa == pb and _same(ia, ib)
    for imgs, paths in plain:                                            # and both are today's definition
        for k, path in enumerate(paths):
            assert _same(imgs[k], _want(path, None, False, demosaic)), path


def test_cli_val_with_calibration_and_sidecars(folder, tmp_path):
    from _synth import synth_state_dict
    from adaptiveisp_amd.agent import Agent
    from adaptiveisp_amd.config import cfg
    agent = Agent(cfg, shape=(6 + len(cfg.filters), 64, 64))
    torch.save({"iter": 0, "agent_model": synth_state_dict(agent, seed=0)}, tmp_path / "agent.pth")
    cmd = ["timeout", "-k", "10", "300", sys.executable, "-m", "adaptiveisp_amd.val", "--isp-ckpt", str(tmp_path / "agent.pth"),
           "--data", str(folder / "images"), "--data-name", "raw", "--cfa", CFA, "--raw-bits", "12", "--demosaic", "mhc",
           "--raw-cal", str(folder / "cal.npz"), "--raw-meta", "--raw-dpc", "25", "--img-size", str(S), "--batch-size", "2",
           "--steps", "1", "--project", str(tmp_path / "runs"), "--name", "rawfix"]
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    r = subprocess.run(cmd, cwd=ROOT, env=env, capture_output=True, text=True)         # a fresh child process
    assert r.returncode == 0, f"exit {r.returncode}\n{r.stdout[-3000:]}\n{r.stderr[-3000:]}"
    run = r.stdout.strip().splitlines()[-1].split("Results saved to ", 1)[1]
    res = json.load(open(os.path.join(run, "results.json")))
    assert os.path.isfile(os.path.join(run, "records.txt")) and res["seen"] == 4
    assert res["args"]["raw_cal"] == str(folder / "cal.npz") and res["args"]["raw_meta"] is True and res["args"]["raw_dpc"] == 25
    assert "cal.npz" in r.stdout and "dpc 25" in r.stdout and "3 sidecars" in r.stdout
