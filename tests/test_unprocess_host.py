"""Host side of the image-dataset replay source (adaptiveisp_amd/data.py) and the C entry adaisp_unprocess, without a GPU:
the metadata draws against the reference (tests/golden/unprocess.npz), the float64 restatement the GPU tests lean on,
file order / sharding / labels / prefetch of ImageFolderSource, and the argument checks of the C entry."""
import ctypes
import random

import numpy as np
import pytest
import torch

import _unprocessref as U
from adaptiveisp_amd import _lib
from adaptiveisp_amd.data import ImageFolderSource, kernel_params, sample_unprocess_params
from adaptiveisp_amd.val.loader import LODImages

SIZES = [(40, 30), (17, 50), (64, 64), (33, 21), (80, 12), (9, 71), (25, 25)]


def _case(z, k):
    c = f"case{k}."
    bri = tuple(z[c + "bri"]) if not np.isnan(z[c + "bri"]).any() else None
    level = None if np.isnan(z[c + "noise_level"]) else float(z[c + "noise_level"])
    return (int(z[c + "seed"]), bool(z[c + "add_noise"]), bri, level, bool(z[c + "use_linear"]),
            z[f"img{int(z[c + 'img'])}"])


def _ncases(z):
    return len([f for f in z.files if f.startswith("case") and f.endswith(".out")])


def test_fixture_covers_the_options(golden):
    z = golden("unprocess")
    cases = [_case(z, k) for k in range(_ncases(z))]
    assert {c[1] for c in cases} == {False, True}
    assert {c[2] is None for c in cases} == {False, True}
    assert {c[3] is None for c in cases if c[1]} == {False, True}
    assert {c[4] for c in cases if c[1]} == {False, True}


def test_sample_params_reproduce_reference_metadata(golden):
    z = golden("unprocess")
    for k in range(_ncases(z)):
        seed, noise, bri, level, lin, _ = _case(z, k)
        m = sample_unprocess_params(np.random.RandomState(seed), noise, bri, level, lin)
        c = f"case{k}."
        assert np.array_equal(m["rgb2cam"], z[c + "rgb2cam"]), k
        assert (m["rgb_gain"], m["red_gain"], m["blue_gain"]) == tuple(z[c + "gains"]), k
        assert m["gain"] == z[c + "gain"], k
        assert (m["shot"], m["read"]) == tuple(z[c + "noise"]), k


def test_float64_restatement_matches_reference(golden):
    z = golden("unprocess")
    for k in range(_ncases(z)):
        seed, noise, bri, level, lin, img = _case(z, k)
        c = f"case{k}."
        g = z[c + "gains"]
        out = U.unprocess_clean(img, z[c + "rgb2cam"], *g, prescale=0.9, ratio=float(z[c + "gain"]))
        np.testing.assert_allclose(out, z[c + "out"], rtol=0, atol=1e-12, err_msg=f"case {k}")
    out = U.unprocess_clean(z["sat.img"], z["sat.rgb2cam"], *z["sat.gains"], prescale=1.0)
    np.testing.assert_allclose(out, z["sat.out"], rtol=0, atol=1e-12)
    mask = U.saturation_mask(z["sat.img"], z["sat.rgb2cam"])
    assert (mask > 0.05).sum() >= 10 and (mask == 0).any()       # the mask is reached, and not everywhere


def test_kernel_params_layout():
    m = sample_unprocess_params(np.random.RandomState(3), True, (0.1, 0.3), None, False)
    p = kernel_params(m)
    assert p.dtype == np.float32 and p.shape == (16,)
    assert np.array_equal(p[:9], m["rgb2cam"].reshape(-1).astype(np.float32))
    g = np.array([1 / m["red_gain"], 1.0, 1 / m["blue_gain"]]) / m["rgb_gain"]
    assert np.array_equal(p[9:12], g.astype(np.float32))
    assert tuple(p[12:]) == tuple(np.float32([0.9, m["gain"], m["shot"], m["read"]]))


def test_u8_over_255_is_one_rounding():
    u = np.arange(256)
    assert np.array_equal((u / 255.0).astype(np.float32), u.astype(np.float32) / np.float32(255.0))
    assert torch.equal(torch.from_numpy(u.astype(np.uint8)).float() / 255.0, torch.from_numpy((u / 255.0).astype(np.float32)))


def test_philox_known_answers():
    # Random123's published known-answer vectors of philox4x32_10
    assert U.philox4x32_10((0, 0, 0, 0), (0, 0)) == (0x6627E8D5, 0xE169C58D, 0xBC57AC4C, 0x9B00DBD8)
    assert U.philox4x32_10((0xFFFFFFFF,) * 4, (0xFFFFFFFF,) * 2) == (0x408F276D, 0x41C83B0E, 0xA20BC7C6, 0x6D5451FD)
    assert U.philox4x32_10((0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344), (0xA4093822, 0x299F31D0)) == \
        (0xD16CFE09, 0x94FDCCEB, 0x5001E420, 0x24126EA1)


# ---------------------------------------------------------------------------------------------------- ImageFolderSource
@pytest.fixture(scope="module")
def dataset(tmp_path_factory):
    root = tmp_path_factory.mktemp("toyds")
    files = U.write_dataset(str(root), SIZES, seed=5)
    return str(root), files


def _drain(src, sizes):
    out = []
    for n in sizes:
        ims, labels, paths, shapes = src.get_next_batch(n)
        assert len(ims) == len(labels) == len(paths) == len(shapes) == n
        out += list(zip(ims, labels, paths, shapes))
    return out


def _expected_order(n, seed, rank, count):
    rng = random.Random(1000 * seed + rank)
    order = list(range(n))
    while len(order) < count:
        idx = list(range(n))
        rng.shuffle(idx)
        order += idx
    return order[:count]


@pytest.mark.parametrize("seed", [0, 3])
def test_order_first_pass_then_reshuffle(dataset, seed):
    root, files = dataset
    src = ImageFolderSource(root, 32, "cpu", seed=seed, workers=0)
    assert src.files == files
    got = [it[2] for it in _drain(src, [3, 5, 4, 7, 2, 8])]
    assert got == [files[i] for i in _expected_order(len(files), seed, 0, len(got))]
    assert got[:len(files)] == files


def test_txt_list_is_sorted(dataset, tmp_path):
    root, files = dataset
    lst = tmp_path / "list.txt"
    lst.write_text("\n".join(reversed(files)) + "\n")
    assert ImageFolderSource(str(lst), 32, "cpu", workers=0).files == files


@pytest.mark.parametrize("world", [2, 3])
def test_rank_sharding(dataset, world):
    root, files = dataset
    seen = []
    for r in range(world):
        src = ImageFolderSource(root, 32, "cpu", seed=1, rank=r, world=world, workers=0)
        assert src.files == files[r::world]
        got = [it[2] for it in _drain(src, [4, 4])]
        assert got == [src.files[i] for i in _expected_order(len(src.files), 1, r, 8)]
        seen += src.files
    assert sorted(seen) == files


@pytest.mark.parametrize("S", [32, 64, 100])
def test_lod_cpu_bit_equal_to_lodimages(dataset, S):
    root, files = dataset
    ref = LODImages(root, S)
    src = ImageFolderSource(root, S, "cpu", data_name="lod", workers=0)
    for i, (im, label, path, shapes) in enumerate(_drain(src, [4, 3])):
        r_im, r_lb, r_path, r_shapes = ref.item(i)
        assert path == r_path and shapes == r_shapes
        assert im.dtype == torch.float32 and tuple(im.shape) == (3, S, S)
        assert torch.equal(im, r_im), path
        assert label.dtype == np.float32 and label.shape == (len(r_lb), 6)
        assert (label[:, 0] == 0).all() and np.array_equal(label[:, 1:], r_lb)
    assert any(len(r[1]) == 0 for r in map(ref.item, range(len(files))))      # one image has no label file


def test_prefetch_does_not_change_the_sequence(dataset):
    root, _ = dataset
    a = ImageFolderSource(root, 48, "cpu", seed=2, workers=0)
    b = ImageFolderSource(root, 48, "cpu", seed=2, workers=4)
    try:
        for x, y in zip(_drain(a, [3, 5, 6, 4, 8]), _drain(b, [3, 5, 6, 4, 8])):
            assert x[2] == y[2] and x[3] == y[3] and np.array_equal(x[1], y[1]) and torch.equal(x[0], y[0])
    finally:
        b.close()


def test_coco_on_cpu_raises(dataset):
    root, _ = dataset
    with pytest.raises(RuntimeError, match="no CPU path"):
        ImageFolderSource(root, 32, "cpu", data_name="coco", add_noise=True)
    with pytest.raises(ValueError):
        ImageFolderSource(root, 32, "cpu", data_name="raw")


# ---------------------------------------------------------------------------------------------------- C entry, no GPU
def test_cabi_unprocess_rejects_bad_arguments():
    L = _lib.load()
    p = ctypes.c_void_p(4096)                         # never dereferenced: every call below fails its checks first
    E = -1
    assert L.adaisp_unprocess(None, p, p, 1, 8, 0, 0, None) == E
    assert L.adaisp_unprocess(p, None, p, 1, 8, 0, 0, None) == E
    assert L.adaisp_unprocess(p, p, None, 1, 8, 0, 0, None) == E
    assert L.adaisp_unprocess(p, p, p, 0, 8, 0, 0, None) == E
    assert L.adaisp_unprocess(p, p, p, -3, 8, 0, 0, None) == E
    assert L.adaisp_unprocess(p, p, p, 1, 0, 0, 0, None) == E
    assert L.adaisp_unprocess(p, p, p, 1, -1, 0, 0, None) == E
    assert L.adaisp_unprocess(p, p, p, 1, 8, 0, 4, None) == E                    # unknown flag bit
    assert L.adaisp_unprocess(p, p, p, 1, 8, 0, 0x80000000, None) == E
    assert L.adaisp_unprocess(p, p, p, 1, 8, 0, _lib.UNP_NOISE, None) == E       # noise without the unprocess
    assert L.adaisp_unprocess(p, p, p, 65536, 8, 0, 0, None) == -4
    assert L.adaisp_unprocess(p, p, p, 1, 32769, 0, 0, None) == -4
    assert "adaisp_unprocess" in _lib.EXPORTS
    assert _lib.UNPROCESS_DESC.itemsize == 96
    assert [_lib.UNPROCESS_DESC.fields[f][1] for f in ("src_offset", "h", "w", "top", "left", "serial", "p")] == \
        [0, 8, 12, 16, 20, 24, 32]


def test_wrapper_rejects_host_tensors():
    with pytest.raises(_lib.AdaispError, match="device"):
        _lib.unprocess(torch.zeros(12, dtype=torch.uint8), torch.zeros(96, dtype=torch.uint8), 2)
