"""Image datasets as the RL trainer's replay source (the reference's two replay loaders, replay_memory.py:60-97):

  `lod`   LoadImagesAndLabelsNormalizeReplay (dataset.py:794-897): decode, longer side to S, letterbox to S x S with
          black, /255.
  `coco`  LoadImagesAndLabelsRAWReplay (dataset.py:420-561): the sRGB image becomes synthetic low-light linear RGB by
          `unprocess_wo_mosaic` (isp/unprocess_np.py:248-292) before the letterbox.

Decoding and resizing run on the host in `workers` threads; only the un-padded uint8 image crosses PCIe (3 B/px instead
of the reference's fp32 / fp64), and one adaisp_unprocess launch per batch converts, unprocesses, adds the noise and
letterboxes on the device. The random draws of the metadata are the reference's, in its order
(`sample_unprocess_params`); the per-sample normals come from a counter-based generator on the device, so the noise is
equal to the reference's in distribution, not in value.
"""
import random
from collections import deque
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import torch

from .val.loader import list_images, load_letterboxed

# random_ccm's XYZ -> camera matrices and the sRGB RGB -> XYZ matrix (isp/unprocess_np.py:5-35; Brooks et al.,
# "Unprocessing Images for Learned Raw Denoising", CVPR 2019)
XYZ2CAMS = np.array([[[1.0234, -0.2969, -0.2266], [-0.5625, 1.6328, -0.0469], [-0.0703, 0.2188, 0.6406]],
                     [[0.4913, -0.0541, -0.0202], [-0.613, 1.3513, 0.2906], [-0.1564, 0.2151, 0.7183]],
                     [[0.838, -0.263, -0.0639], [-0.2887, 1.0725, 0.2496], [-0.0627, 0.1427, 0.5438]],
                     [[0.6596, -0.2079, -0.0562], [-0.4782, 1.3016, 0.1933], [-0.097, 0.1581, 0.5181]]])
RGB2XYZ = np.array([[0.4124564, 0.3575761, 0.1804375], [0.2126729, 0.7151522, 0.0721750], [0.0193339, 0.1191920, 0.9503041]])
PRESCALE = 0.9          # unprocess_wo_mosaic's adjust_random_brightness(image, s_range=0.9)


def sample_unprocess_params(rs, add_noise=False, brightness_range=None, noise_level=None, use_linear=False):
    """The metadata draws of one `unprocess_wo_mosaic` call from the np.random.RandomState `rs`, in the reference's order:
    random_ccm (uniform (4,1,1)), random_gains (normal, uniform, uniform), the brightness ratio (rand, if
    `brightness_range`), the noise levels (if `add_noise`: a log-uniform or uniform shot draw unless `noise_level` gives it,
    then normal(0, 0.26)). Returns dict(rgb2cam [3,3], rgb_gain, red_gain, blue_gain, gain, shot, read), float64.

    It does NOT make the per-sample normal draw of add_read_and_shot_noise (the device draws those): with the same seed the
    metadata of the first image is bit-identical to the reference's, and the two sequences diverge after the first noisy
    image, whose H*W*3 normals the reference takes from the same stream."""
    weights = rs.uniform(1e-8, 1e8, size=(len(XYZ2CAMS), 1, 1))
    xyz2cam = np.sum(XYZ2CAMS * weights, axis=0) / np.sum(weights, axis=0)
    rgb2cam = np.matmul(xyz2cam, RGB2XYZ)
    rgb2cam = rgb2cam / np.sum(rgb2cam, axis=-1, keepdims=True)
    rgb_gain = 1.0 / rs.normal(0.8, 0.1)
    red_gain = rs.uniform(1.9, 2.4)
    blue_gain = rs.uniform(1.5, 1.9)
    gain = 1.0
    if brightness_range is not None:
        if isinstance(brightness_range, (list, tuple)):
            lo, hi = brightness_range
            assert lo < hi, "brightness_range[0] should be less than brightness_range[1]"
            gain = rs.rand() * (hi - lo) + lo
        else:
            gain = brightness_range
    shot = read = 0.0
    if add_noise:
        if noise_level is not None:
            shot = noise_level
            log_shot = np.log(shot)
        elif use_linear:
            shot = rs.uniform(0.0001, 0.012)
            log_shot = np.log(shot)
        else:
            log_shot = rs.uniform(np.log(0.0001), np.log(0.012))
            shot = np.exp(log_shot)
        read = np.exp(2.18 * log_shot + 1.20 + rs.normal(0, 0.26))
    return dict(rgb2cam=rgb2cam, rgb_gain=rgb_gain, red_gain=red_gain, blue_gain=blue_gain, gain=gain, shot=shot, read=read)


def kernel_params(meta, prescale=PRESCALE):
    """The 16 adaisp_unprocess parameters (ADAISP_UNP_* slots of include/adaisp.h) of one metadata dict, float32."""
    p = np.zeros(16, np.float32)
    p[0:9] = meta["rgb2cam"].reshape(-1)
    p[9:12] = np.stack((1.0 / meta["red_gain"], 1.0, 1.0 / meta["blue_gain"])) / meta["rgb_gain"]
    p[12], p[13], p[14], p[15] = prescale, meta["gain"], meta["shot"], meta["read"]
    return p


class ImageFolderSource:
    """The DeviceReplayMemory source contract over an image dataset: get_next_batch(n) -> (images [n,3,S,S] on `device`,
    labels [k,6] float32 (column 0 zero), paths, shapes), the reference's `get_next_batch_` (dataset.py:541-561).

    Files: a directory or a .txt list, sorted as LoadImagesAndLabels does (dataloaders.py:482); rank r of `world` takes
    files[r::world]. Order: the first pass in file order, every wrap reshuffled with the source's own
    random.Random(1000 * seed + rank) (with world = 1 the reference's draw order). Metadata draws: np.random.RandomState of
    the same seed, one sample_unprocess_params per image in delivery order; noise key (1000 * seed + rank, image serial),
    the serial counting the images this source has delivered.

    Decoding: val/loader.load_letterboxed (load_image's area filter when shrinking; letterbox geometry with auto=False,
    scaleup=False, colour 0). The one ordering difference from the reference: when the letterbox must resize (a one-pixel
    ceil overshoot of load_image) the uint8 image is resized on the host BEFORE the unprocess; the reference resizes the
    unprocessed float image. `workers` threads decode ahead (0: on the calling thread); the delivered sequence is the same
    for every worker count. Only the calling thread touches the device: it fills a pinned staging slot (reused only after
    the event of its previous copy has completed), issues one H2D copy of descriptors + pixels and one adaisp_unprocess
    launch on the current stream.

    On a CPU device `lod` is computed by torch exactly as LODImages does; `coco` has no CPU path and raises."""

    def __init__(self, source, img_size, device, data_name="lod", add_noise=False, brightness_range=None, noise_level=None,
                 use_linear=False, seed=0, rank=0, world=1, workers=4):
        if data_name not in ("lod", "coco"):
            raise ValueError(f"data_name must be 'lod' or 'coco', got {data_name!r}")
        self.device = torch.device(device)
        if data_name == "coco" and self.device.type != "cuda":
            raise RuntimeError("ImageFolderSource(data_name='coco'): the unprocess runs on the HIP device only "
                               "(adaisp_unprocess); there is no CPU path")
        if add_noise and data_name != "coco":
            raise ValueError("add_noise needs data_name='coco'")
        if brightness_range is not None and isinstance(brightness_range, (list, tuple)):
            brightness_range = tuple(float(v) for v in brightness_range)
        self.files = sorted(list_images(source))[rank::world]
        if not self.files:
            raise FileNotFoundError(f"{source}: no images for rank {rank} of {world}")
        self.img_size, self.data_name = int(img_size), data_name
        self.add_noise, self.brightness_range = bool(add_noise), brightness_range
        self.noise_level, self.use_linear = noise_level, bool(use_linear)
        self.seed = 1000 * int(seed) + int(rank)
        self.rng = random.Random(self.seed)
        self.rs = np.random.RandomState(self.seed)
        self.indices = list(range(len(self.files)))
        self.serial = 0
        self.workers = int(workers)
        self._pool = ThreadPoolExecutor(max_workers=self.workers) if self.workers > 0 else None
        self._ahead = deque()                     # (index, Future | decoded item), in delivery order
        self._slots = [dict(host=None, event=None) for _ in range(2)]
        self._slot = 0
        self._dev = None

    def __len__(self):
        return len(self.files)

    def close(self):
        if self._pool is not None:
            self._pool.shutdown(wait=True, cancel_futures=True)
            self._pool = None

    def describe(self):
        kind = "coco (unprocess" + (", noise" if self.add_noise else "") + ")" if self.data_name == "coco" else "lod"
        return f"{kind}: {len(self.files)} files"

    # ------------------------------------------------------------------------------------------------------ order
    def _next_index(self):
        i = self.indices[0]
        self.indices = self.indices[1:]
        if not self.indices:
            self.indices = list(range(len(self.files)))
            self.rng.shuffle(self.indices)
        return i

    def _decode(self, i):
        im, (top, left), _, lb, shapes = load_letterboxed(self.files[i], self.img_size)
        label = np.zeros((len(lb), 6), np.float32)
        label[:, 1:] = lb
        return im, top, left, label, self.files[i], shapes

    def _take(self, n):
        """The next n decoded items; with workers, keeps up to 2 * n more decoding behind them."""
        if self._pool is None:
            return [self._decode(self._next_index()) for _ in range(n)]
        while len(self._ahead) < 2 * n:
            i = self._next_index()
            self._ahead.append(self._pool.submit(self._decode, i))
        return [self._ahead.popleft().result() for _ in range(n)]

    # ------------------------------------------------------------------------------------------------------ batches
    def get_next_batch(self, n):
        n = int(n)
        items = self._take(n)
        labels, paths, shapes = [it[3] for it in items], [it[4] for it in items], [it[5] for it in items]
        if self.device.type != "cuda":
            return list(self._cpu_lod(items)), labels, paths, shapes
        return list(self._device_batch(items)), labels, paths, shapes

    def _cpu_lod(self, items):
        S = self.img_size
        out = torch.zeros((len(items), 3, S, S))
        for b, (im, top, left, *_rest) in enumerate(items):
            chw = np.ascontiguousarray(im.transpose(2, 0, 1)[::-1])
            out[b, :, top:top + im.shape[0], left:left + im.shape[1]] = torch.from_numpy(chw).float() / 255.0
        return out.to(self.device)

    def _device_batch(self, items):
        from . import _lib
        S, B = self.img_size, len(items)
        desc = np.zeros(B, _lib.UNPROCESS_DESC)
        dbytes = (B * _lib.UNPROCESS_DESC.itemsize + 15) // 16 * 16
        off = 0
        for b, (im, top, left, *_rest) in enumerate(items):
            desc[b]["src_offset"], desc[b]["h"], desc[b]["w"] = off, im.shape[0], im.shape[1]
            desc[b]["top"], desc[b]["left"], desc[b]["serial"] = top, left, self.serial
            self.serial += 1
            off += im.size
        flags = 0
        if self.data_name == "coco":
            flags = _lib.UNP_UNPROCESS | (_lib.UNP_NOISE if self.add_noise else 0)
            for b in range(B):
                desc[b]["p"] = kernel_params(sample_unprocess_params(self.rs, self.add_noise, self.brightness_range,
                                                                     self.noise_level, self.use_linear))
        total = dbytes + off
        slot = self._slots[self._slot]
        self._slot = (self._slot + 1) % len(self._slots)
        if slot["event"] is not None:
            slot["event"].synchronize()           # this slot's previous H2D copy has finished reading it
        if slot["host"] is None or slot["host"].numel() < total:
            slot["host"] = torch.empty(max(total, dbytes + B * S * S * 3), dtype=torch.uint8, pin_memory=True)
        host = slot["host"].numpy()
        host[:B * desc.itemsize] = desc.view(np.uint8)
        pos = dbytes
        for im, *_rest in items:
            host[pos:pos + im.size] = im.reshape(-1)
            pos += im.size
        with torch.cuda.device(self.device):
            if self._dev is None or self._dev.numel() < total:
                self._dev = torch.empty(slot["host"].numel(), dtype=torch.uint8, device=self.device)
            self._dev[:total].copy_(slot["host"][:total], non_blocking=True)
            slot["event"] = torch.cuda.Event()
            slot["event"].record()
            return _lib.unprocess(self._dev[dbytes:total], self._dev[:B * desc.itemsize], S, seed=self.seed, flags=flags)
