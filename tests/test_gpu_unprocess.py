"""adaisp_unprocess on the MI355X (csrc/isp_unprocess.hip) and the image-dataset replay source feeding the RL trainer
(adaptiveisp_amd/data.py): the convert mode bit for bit against LODImages, the unprocess chain against the reference's
fixture (tests/golden/unprocess.npz) and the float64 restatement (tests/_unprocessref.py) at ragged shapes, the letterbox pad
and the output bounds, the noise's determinism and statistics, and the trainer / CLI end to end."""
import json
import os
import random
import subprocess
import sys

import numpy as np
import pytest
import torch

import _unprocessref as U
from adaptiveisp_amd import _lib
from adaptiveisp_amd.data import ImageFolderSource, kernel_params, sample_unprocess_params
from adaptiveisp_amd.val.loader import LODImages, load_letterboxed

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# |fp32 kernel - float64 restatement| of the noise-free unprocess, 4x the largest error measured on the MI355X: 1.63e-7
# over the shapes below at 6 parameter draws each and the fixture's cases; 1.02e-6 on the saturation case, where the mask's
# (gray - 0.9) / 0.1 amplifies the fp32 rounding of the colour matrix
TOL = 4 * 1.64e-7
TOL_SAT = 4 * 1.02e-6


def _params(seed, prescale=0.9, bri=None, noise=False, level=None, lin=False):
    m = sample_unprocess_params(np.random.RandomState(seed), noise, bri, level, lin)
    return m, kernel_params(m, prescale)


def _launch(imgs, place, S, flags=0, params=None, serials=None, seed=0, gap=0, out=None):
    """imgs: uint8 HWC BGR arrays; place: (top, left) each. `gap` bytes between images (odd: odd source offsets)."""
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
    d = torch.from_numpy(desc.view(np.uint8).copy()).to(DEV)
    r = _lib.unprocess(src, d, S, seed=seed, flags=flags, out=out)
    torch.cuda.synchronize()
    return r


def _expected_convert(im, S, top, left):
    chw = torch.from_numpy(np.ascontiguousarray(im.transpose(2, 0, 1)[::-1])).float() / 255.0
    out = torch.zeros(3, S, S)
    out[:, top:top + im.shape[0], left:left + im.shape[1]] = chw
    return out


def _rand_u8(rs, h, w, lo=0, hi=256):
    im = rs.randint(lo, hi, size=(h, w, 3)).astype(np.uint8)
    if lo == 0 and hi == 256:
        im.reshape(-1)[0], im.reshape(-1)[-1] = 0, 255
    return im


# (h, w, S, top, left)
SHAPES = [(1, 1, 1, 0, 0), (1, 1, 8, 3, 5), (3, 5, 7, 1, 1), (3, 5, 16, 0, 11), (37, 511, 512, 237, 0),
          (512, 512, 512, 0, 0), (511, 40, 512, 1, 235), (40, 511, 512, 235, 1), (29, 33, 37, 3, 1), (64, 17, 64, 0, 23)]


@pytest.mark.parametrize("h,w,S,top,left", SHAPES)
def test_shapes_convert_exact_and_unprocess_close(h, w, S, top, left):
    rs = np.random.RandomState(h * 1000 + w)
    im = _rand_u8(rs, h, w)
    got = _launch([im], [(top, left)], S, gap=(w % 2) + 1).cpu()[0]
    assert torch.equal(got, _expected_convert(im, S, top, left))
    m, p = _params(h + w)
    got = _launch([im], [(top, left)], S, _lib.UNP_UNPROCESS, [p], gap=3).cpu().numpy()[0]
    ref = U.letterboxed(U.unprocess_clean(im, m["rgb2cam"], m["rgb_gain"], m["red_gain"], m["blue_gain"]), S, top, left)
    assert np.abs(got - ref).max() <= TOL
    pad = np.ones((S, S), bool)
    pad[top:top + h, left:left + w] = False
    assert (got[:, pad] == 0).all()


def test_mixed_batch_of_eight_with_odd_offsets():
    rs = np.random.RandomState(8)
    S = 96
    dims = [(96, 96), (1, 1), (95, 3), (3, 95), (50, 77), (77, 50), (13, 96), (96, 13)]
    imgs = [_rand_u8(rs, h, w) for h, w in dims]
    place = [(0, 0), (95, 95), (1, 47), (46, 1), (23, 9), (9, 23), (41, 0), (0, 41)]
    ps = [_params(20 + b, bri=(0.1, 0.3)) for b in range(8)]
    conv = _launch(imgs, place, S, gap=5).cpu()
    unp = _launch(imgs, place, S, _lib.UNP_UNPROCESS, [p for _, p in ps], gap=7).cpu().numpy()
    for b in range(8):
        assert torch.equal(conv[b], _expected_convert(imgs[b], S, *place[b])), b
        m = ps[b][0]
        ref = U.letterboxed(U.unprocess_clean(imgs[b], m["rgb2cam"], m["rgb_gain"], m["red_gain"], m["blue_gain"],
                                              ratio=m["gain"]), S, *place[b])
        assert np.abs(unp[b] - ref).max() <= TOL, b


def test_unprocess_matches_reference_fixture(golden):
    z = golden("unprocess")
    k = 0
    while f"case{k}.out" in z.files:
        c = f"case{k}."
        img = z[f"img{int(z[c + 'img'])}"]
        m = dict(rgb2cam=z[c + "rgb2cam"], rgb_gain=z[c + "gains"][0], red_gain=z[c + "gains"][1],
                 blue_gain=z[c + "gains"][2], gain=float(z[c + "gain"]), shot=0.0, read=0.0)
        S = max(img.shape[:2]) + 3
        got = _launch([img], [(1, 2)], S, _lib.UNP_UNPROCESS, [kernel_params(m)]).cpu().numpy()[0]
        ref = U.letterboxed(z[c + "out"], S, 1, 2)
        assert np.abs(got - ref).max() <= TOL, k
        k += 1
    assert k >= 8
    # pre-scale 1.0 on near-white pixels: safe_invert_gains' mask is reached
    g = z["sat.gains"]
    m = dict(rgb2cam=z["sat.rgb2cam"], rgb_gain=g[0], red_gain=g[1], blue_gain=g[2], gain=1.0, shot=0.0, read=0.0)
    img = z["sat.img"]
    assert (U.saturation_mask(img, z["sat.rgb2cam"]) > 0.05).sum() >= 10
    got = _launch([img], [(0, 0)], max(img.shape[:2]), _lib.UNP_UNPROCESS, [kernel_params(m, 1.0)]).cpu().numpy()[0]
    ref = U.letterboxed(z["sat.out"], max(img.shape[:2]), 0, 0)
    assert np.abs(got - ref).max() <= TOL_SAT


@pytest.mark.parametrize("flags", [0, _lib.UNP_UNPROCESS, _lib.UNP_UNPROCESS | _lib.UNP_NOISE])
@pytest.mark.parametrize("S,misalign", [(64, 0), (64, 1), (37, 0)])
def test_pad_and_bounds(flags, S, misalign):
    """A NaN-prefilled output is written everywhere, the pad is exactly 0, and sentinels past B*3*S*S (and before a
    misaligned start: the scalar-store path) stay as they were."""
    rs = np.random.RandomState(S)
    imgs = [_rand_u8(rs, 20, S), _rand_u8(rs, S, 9), _rand_u8(rs, 1, 1)]
    place = [(5, 0), (0, S - 9), (S - 1, 0)]
    params = [_params(b, noise=True)[1] for b in range(3)]
    n = 3 * 3 * S * S
    buf = torch.full((n + 4096 + misalign,), float("nan"), device=DEV)
    buf[:misalign] = 1234.5
    buf[misalign + n:] = -777.0
    out = buf[misalign:misalign + n].view(3, 3, S, S)
    _launch(imgs, place, S, flags, params, out=out)
    b = buf.cpu()
    assert (b[:misalign] == 1234.5).all() and (b[misalign + n:] == -777.0).all()
    o = out.cpu().numpy()
    assert np.isfinite(o).all() and (o >= 0).all() and (o <= 1).all()
    for i, (im, (top, left)) in enumerate(zip(imgs, place)):
        pad = np.ones((S, S), bool)
        pad[top:top + im.shape[0], left:left + im.shape[1]] = False
        assert (o[i][:, pad] == 0).all()


def test_a_placement_outside_the_frame_gives_zeros():
    rs = np.random.RandomState(1)
    im = _rand_u8(rs, 10, 10)
    got = _launch([im, im, im], [(0, 0), (7, 0), (0, -1)], 16).cpu()
    assert torch.equal(got[0], _expected_convert(im, 16, 0, 0))
    assert (got[1:] == 0).all()


# ------------------------------------------------------------------------------------------------------------ noise
SHOT, READ = 0.001, 1e-5       # with pixels 120..255 every clean sample lies in [6 sigma, 1 - 6 sigma]


def _noise_case(B=1, h=200, w=300):
    rs = np.random.RandomState(5)
    imgs = [_rand_u8(rs, h, w, 120, 256) for _ in range(B)]
    params = []
    for b in range(B):
        _, p = _params(b)
        p[14], p[15] = SHOT, READ
        params.append(p)
    return imgs, params


def test_noise_is_a_function_of_seed_and_serial():
    imgs, params = _noise_case(B=8, h=60, w=70)
    NF = _lib.UNP_UNPROCESS | _lib.UNP_NOISE
    place = [(b, b + 1) for b in range(8)]
    a = _launch(imgs, place, 80, NF, params, serials=list(range(100, 108)), seed=7, gap=3).cpu()
    b = _launch(imgs, place, 80, NF, params, serials=list(range(100, 108)), seed=7, gap=3).cpu()
    assert torch.equal(a, b)
    # image 5 alone, at another offset and placement, is the same image
    alone = _launch([imgs[5]], [(0, 0)], 70, NF, [params[5]], serials=[105], seed=7, gap=0).cpu()
    t, l = place[5]
    assert torch.equal(alone[0, :, :60, :70], a[5, :, t:t + 60, l:l + 70])
    c = _launch(imgs, place, 80, NF, params, serials=list(range(100, 108)), seed=8, gap=3).cpu()
    assert not torch.equal(a, c)
    # the draws are the restated Philox4x32-10 + Box-Muller ones
    clean = _launch([imgs[5]], [(0, 0)], 70, _lib.UNP_UNPROCESS, [params[5]]).cpu().numpy()[0]
    sig = np.sqrt(clean.astype(np.float64) * SHOT + READ)
    z = (alone.numpy()[0].astype(np.float64) - clean) / sig
    for idx in (0, 1, 69, 70, 1234, 60 * 70 - 1):
        y, x = divmod(idx, 70)
        ref = U.normals3(7, 105, idx)
        ok = (clean[:, y, x] > 6 * sig[:, y, x]) & (clean[:, y, x] < 1 - 6 * sig[:, y, x])
        assert np.abs(z[:, y, x] - ref)[ok].max(initial=0) < 2e-3, (idx, z[:, y, x], ref)


def test_noise_of_different_serials_is_uncorrelated():
    imgs, params = _noise_case(B=1, h=400, w=400)
    NF = _lib.UNP_UNPROCESS | _lib.UNP_NOISE
    clean = _launch(imgs, [(0, 0)], 400, _lib.UNP_UNPROCESS, params).cpu().numpy()[0].astype(np.float64)
    n1 = _launch(imgs, [(0, 0)], 400, NF, params, serials=[1], seed=3).cpu().numpy()[0] - clean
    n2 = _launch(imgs, [(0, 0)], 400, NF, params, serials=[2], seed=3).cpu().numpy()[0] - clean
    n3 = _launch(imgs, [(0, 0)], 400, NF, params, serials=[1 << 32 | 1], seed=3).cpu().numpy()[0] - clean
    for a, b in ((n1, n2), (n1, n3)):
        assert abs(np.corrcoef(a.reshape(-1), b.reshape(-1))[0, 1]) < 0.01
    # the three channels of one pixel are independent draws
    assert abs(np.corrcoef(n1[0].reshape(-1), n1[1].reshape(-1))[0, 1]) < 0.01
    assert abs(np.corrcoef(n1[0].reshape(-1), n1[2].reshape(-1))[0, 1]) < 0.01


def test_noise_statistics():
    imgs, params = _noise_case(B=4, h=512, w=512)
    place = [(0, 0)] * 4
    NF = _lib.UNP_UNPROCESS | _lib.UNP_NOISE
    clean = _launch(imgs, place, 512, _lib.UNP_UNPROCESS, params).cpu().numpy().astype(np.float64)
    noisy = _launch(imgs, place, 512, NF, params, serials=[11, 12, 13, 14], seed=1).cpu().numpy()
    assert (noisy >= 0).all() and (noisy <= 1).all()
    sig = np.sqrt(clean * SHOT + READ)
    ok = (clean >= 6 * sig) & (clean <= 1 - 6 * sig)
    z = ((noisy - clean) / sig)[ok]
    assert z.size >= 1_000_000, z.size
    mean, std = z.mean(), z.std()
    kurt = np.mean(((z - mean) / std) ** 4)
    assert abs(mean) <= 0.005 and abs(std - 1) <= 0.005 and abs(kurt - 3) <= 0.05, (mean, std, kurt)


# ------------------------------------------------------------------------------------------------------------ the source
@pytest.fixture(scope="module")
def dataset(tmp_path_factory):
    root = tmp_path_factory.mktemp("gpuds")
    sizes = [(40, 30), (17, 50), (64, 64), (33, 21), (80, 12), (9, 71), (25, 25), (130, 90), (3, 3)]
    files = U.write_dataset(str(root), sizes, seed=9)
    return str(root), files


@pytest.mark.parametrize("S", [64, 100])
def test_lod_source_on_device_is_bit_exact_to_lodimages(dataset, S):
    root, files = dataset
    ref = LODImages(root, S)
    src = ImageFolderSource(root, S, DEV, data_name="lod", workers=2)
    try:
        got = []
        for n in (4, 3, 2):
            ims, labels, paths, shapes = src.get_next_batch(n)
            got += list(zip(ims, labels, paths, shapes))
        torch.cuda.synchronize()
        for i, (im, lb, path, shapes) in enumerate(got):
            r = ref.item(i)
            assert path == r[2] and shapes == r[3] and np.array_equal(lb[:, 1:], r[1])
            assert im.is_cuda and torch.equal(im.cpu(), r[0]), path
    finally:
        src.close()


def test_coco_source_is_the_restated_unprocess(dataset):
    root, files = dataset
    S = 64
    src = ImageFolderSource(root, S, DEV, data_name="coco", brightness_range=(0.2, 0.6), seed=4, workers=0)
    rs = np.random.RandomState(4000)
    ims, _, paths, _ = src.get_next_batch(5)
    ims2, _, paths2, _ = src.get_next_batch(5)
    torch.cuda.synchronize()
    for im, path in zip(ims + ims2, paths + paths2):
        u8, (top, left), _, _, _ = load_letterboxed(path, S)
        m = sample_unprocess_params(rs, False, (0.2, 0.6))
        ref = U.letterboxed(U.unprocess_clean(u8, m["rgb2cam"], m["rgb_gain"], m["red_gain"], m["blue_gain"],
                                              ratio=m["gain"]), S, top, left)
        assert np.abs(im.cpu().numpy() - ref).max() <= TOL, path


def test_noisy_source_reproduces_and_ignores_prefetch(dataset):
    root, _ = dataset
    out = []
    for workers in (0, 3):
        src = ImageFolderSource(root, 64, DEV, data_name="coco", add_noise=True, brightness_range=(0.1, 0.3), seed=2,
                                workers=workers)
        try:
            out.append([torch.stack(src.get_next_batch(n)[0]).cpu() for n in (4, 4, 5)])
        finally:
            src.close()
    for a, b in zip(*out):
        assert torch.equal(a, b)


@pytest.mark.parametrize("mode", [False, True, "split"])
def test_trainer_on_a_noisy_coco_source(dataset, mode):
    from test_gpu_train_graph import _detector, _fresh
    from adaptiveisp_amd.replay import DeviceReplayMemory
    from adaptiveisp_amd.train import Trainer
    from adaptiveisp_amd.util import STATE_STEP_DIM, Dict
    root, _ = dataset
    B, S, N = 4, 64, 12
    eng, loss_fn = _detector(B, S, S)
    cfg, agent, value = _fresh(B)
    c = Dict(cfg)
    c.replay_memory_size = 16
    np.random.seed(0)
    source = ImageFolderSource(root, S, DEV, data_name="coco", add_noise=True, seed=1, workers=2)
    try:
        replay = DeviceReplayMemory(c, source, B, DEV, (3, S, S), rng=random.Random(5))
        tr = Trainer(c, agent, value, eng, loss_fn, replay, batch_size=B, lr=3e-5, epochs=1, graph=mode)
        h = tr.train(iters=N)
        torch.cuda.synchronize()
        assert len(h) == N and all(np.isfinite([r["agent_loss"], r["value_loss"], r["reward"]]).all() for r in h)
        assert len(replay.image_pool) == 16 and len(replay.image_pool) + len(replay.free) == replay.images.shape[0]
        replay.drop_batch(replay.get_next_fake_batch(B))                 # B records leave, B fresh ones are stored
        torch.cuda.synchronize()
        assert len(replay.image_pool) == 16 and len({r.slot for r in replay.image_pool}) == 16
        fresh = [r for r in replay.image_pool if float(r.state[STATE_STEP_DIM]) == 0]
        assert len(fresh) >= B
        pool = replay.images.cpu().numpy()
        for r in fresh:
            u8, (top, left), _, _, _ = load_letterboxed(r.path, S)
            pad = np.ones((S, S), bool)
            pad[top:top + u8.shape[0], left:left + u8.shape[1]] = False
            assert (pool[r.slot][:, pad] == 0).all() and np.isfinite(pool[r.slot]).all()
        assert source.serial >= 16
    finally:
        source.close()


def test_cli_trains_on_a_dataset(dataset):
    root, _ = dataset
    cache = os.path.join(ROOT, "adaptiveisp_amd", "yolo", "tuning", "mi355x.json")
    saved = open(cache, "rb").read()              # the CLI autotunes into the committed table: give it back as it was
    try:
        r = subprocess.run(["timeout", "-k", "10", "600", sys.executable, "-m", "adaptiveisp_amd.train", "--data", root,
                            "--data-name", "coco", "--add-noise", "--bri-range", "0.1", "0.3", "--batch", "2", "--size",
                            "64", "--iters", "4", "--data-workers", "2"], cwd=ROOT, capture_output=True, text=True)
    finally:
        with open(cache, "wb") as f:
            f.write(saved)
    assert r.returncode == 0, r.stderr[-3000:]
    line = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1])
    assert line["data"].startswith("coco (unprocess, noise): 9 files"), line["data"]
    assert line["steps"] == 2 and line["ms_per_iter"] > 0
