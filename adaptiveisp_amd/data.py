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

  `raw`   real captures (no counterpart in the reference, whose raw path starts from a synthesised plane): one 2-D uint16
          .npy colour-filter-array plane per frame at the sensor's size. The plane crosses PCIe as it is (2 B/px) and one
          adaisp_raw_load launch demosaics, applies per-channel gains, resamples to the letterbox size and places it.

sensor="bayer" puts a simulated camera between the two: adaisp_unprocess_bayer keeps the one colour a Bayer filter passes
at every pixel of the unprocessed (and, with add_noise, noisy) image and quantises it to a raw_bits plane, and
adaisp_demosaic_rects interpolates the batch back from that plane, so the noise the policy sees is the demosaiced noise
of a raw sensor rather than white noise per channel (the reference's `unprocess` + `mosaic`, isp/unprocess_np.py:217-245).
"""
import os
import random
from collections import deque
from concurrent.futures import ThreadPoolExecutor
from typing import NamedTuple

import numpy as np
import torch

from .val.loader import (RAW_FORMATS, _label_path, imread_bgr, letterboxed_geometry, letterboxed_labels, list_images,
                         load_image, load_letterboxed, open_raw_plane, read_labels)

# random_ccm's XYZ -> camera matrices and the sRGB RGB -> XYZ matrix (isp/unprocess_np.py:5-35; Brooks et al.,
# "Unprocessing Images for Learned Raw Denoising", CVPR 2019)
XYZ2CAMS = np.array([[[1.0234, -0.2969, -0.2266], [-0.5625, 1.6328, -0.0469], [-0.0703, 0.2188, 0.6406]],
                     [[0.4913, -0.0541, -0.0202], [-0.613, 1.3513, 0.2906], [-0.1564, 0.2151, 0.7183]],
                     [[0.838, -0.263, -0.0639], [-0.2887, 1.0725, 0.2496], [-0.0627, 0.1427, 0.5438]],
                     [[0.6596, -0.2079, -0.0562], [-0.4782, 1.3016, 0.1933], [-0.097, 0.1581, 0.5181]]])
RGB2XYZ = np.array([[0.4124564, 0.3575761, 0.1804375], [0.2126729, 0.7151522, 0.0721750], [0.0193339, 0.1191920, 0.9503041]])
PRESCALE = 0.9          # unprocess_wo_mosaic's adjust_random_brightness(image, s_range=0.9)
AUGMENT_SEED = 0x415547  # added to a source's seed for the two random streams of its augmentation


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


class Item(NamedTuple):
    """One decoded file, as the worker threads hand it to the batch builders. What `pixels`, `size` and `unpad` hold:
      resize="host"     pixels: load_letterboxed's uint8 HWC BGR image, already at its final size; size, unpad: None
      resize="device"   pixels: the decoded uint8 HWC BGR image as it is; size: (h, w) after load_image's resample;
                        unpad: (h2, w2) after letterbox's (letterboxed_geometry): what the device makes of it
      data_name="raw"   pixels: the memory-mapped uint16 plane at the sensor's size; size: as for resize="device", unused
                        (there is no second pass); unpad: the (h2, w2) the plane is resampled to
    (top, left) place the final image in the S x S frame; label is [k,6] float32 with column 0 zero.
    A mosaic tile (mosaic > 0) is load_image's output, not letterboxed: pixels as above but without letterbox's resample
    (unpad == size with resize="device"), top = left = 0, label empty, and `native` holds the file's own rows [k,5]
    (class, x, y, w, h normalised to the image), which load_mosaic places tile by tile."""
    pixels: np.ndarray
    top: int
    left: int
    label: np.ndarray
    path: str
    shapes: tuple
    size: tuple = None
    unpad: tuple = None
    native: np.ndarray = None


class SamplePlan(NamedTuple):
    """The draws of one delivered image of a source with mosaic > 0, made where its index is handed out: `index` the file
    asked for; `mosaics`: () for a single letterboxed image, else one augment.MosaicDraw, or two when mixed up, with `r`
    the mixup ratio (else None); `draw`: an augment.Draw: the whole draw of a single image, and for a mosaic the first
    mosaic's M and s with the image's tables and flips."""
    index: int
    mosaics: tuple
    r: float
    draw: tuple


class Sample(NamedTuple):
    """A SamplePlan and its decoded Items: the letterboxed image, or the 4 (8) tiles in placement order."""
    plan: SamplePlan
    items: list


def _sections(start, *nbytes):
    """Consecutive 16-byte aligned sections of `nbytes` bytes each from `start` on: their offsets, then the aligned end."""
    offsets = []
    for n in nbytes:
        offsets.append(start)
        start = (start + n + 15) // 16 * 16
    return (*offsets, start)


def _label6(rows):
    """Label rows [k,5] as the loaders deliver them: [k,6] float32 with column 0 zero."""
    label = np.zeros((len(rows), 6), np.float32)
    label[:, 1:] = rows
    return label


def _table_index(luts, draw):
    """The index of the Draw's tables in `luts` after appending them (768 bytes), or -1 when it has none."""
    if draw.luts is None:
        return -1
    luts.append(draw.luts.reshape(-1))
    return len(luts) - 1


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

    resize="device" (for photo-sized datasets): the worker threads only decode (and read the labels); the full-size uint8
    image crosses PCIe, with the tap tables of adaptiveisp_amd/resize.py in the same copy, and adaisp_resize_u8 does
    load_image's resample and, for the images whose ceil overshoots, letterbox's bilinear resample on the device, into a
    device scratch that adaisp_unprocess then reads. Same bytes as the host path (the kernel reproduces val/loader.py's
    arithmetic), same metadata draws and noise keys. HIP devices only.

    sensor="bayer" (either data_name, with or without noise, either resize): the same descriptors drive
    adaisp_unprocess_bayer into a reused uint16 device plane (colour filter `cfa`, white level 2**raw_bits - 1,
    `black_level`, default 2**(raw_bits - 6), 0 below 6 bits) and adaisp_demosaic_rects_ex out of it (`demosaic`:
    "bilinear", the default, or "mhc", the 5 x 5 gradient-corrected interpolation, which can leave [0, 1] at edges; it has
    a meaning with sensor="bayer" only and changes nothing before the plane: one seed, one plane); the batch keeps its
    [n,3,S,S] fp32 shape, in [0, 1] over the black..white range. Metadata draws, serials and noise keys are those of
    sensor="rgb": the same seed gives the same sensor parameters in both modes. HIP devices only; an image with a side
    under 2 pixels has no Bayer cell and raises ValueError.

    data_name="raw": the files are .npy, each one 2-D uint16 plane (anything else raises ValueError naming the file, and so
    does a source without any .npy file), labels beside them as for images. Workers only open the file (np.load,
    memory-mapped) and read the labels; the planes are copied from the mappings straight into the pinned slot (by the
    workers, when there are any), each 16-byte aligned, behind the descriptors and tap tables of
    adaptiveisp_amd/resize.RawTapPlan: one H2D copy, one adaisp_raw_load. The plane is resampled from its native size
    straight to letterbox's un-padded size (h2, w2) of letterboxed_geometry (area weights when shrinking, fp32 bilinear
    when enlarging): no second pass for load_image's ceil overshoot. Labels and `shapes` are those of a PNG of the same
    size. `cfa`, `raw_bits`, `black_level`, `demosaic` mean what they mean for sensor="bayer"; `raw_gains` multiplies the
    demosaiced R, G, B; `resize` is accepted and ignored (the resample is always on the device); the unprocess options
    and sensor="bayer" raise ValueError. HIP devices only.
    `raw_calibration` (a rawcal.RawCalibration or the path of one) and `raw_meta` (read <stem>.json beside <stem>.npy when
    the folder is opened: black_level, white_level, gains; a malformed one raises ValueError naming it) are for real
    sensors: with either, adaisp_raw_correct runs before adaisp_raw_load, in a launch of its own over the batch: defect
    pixels, lens shading, per-position black levels, every capture's levels (its sidecar's, else the calibration's, else the
    run's) brought to the run's black_level and white level; a sidecar's gains replace `raw_gains` for that capture.
    Without both, nothing changes: no extra launch, no extra bytes. They raise ValueError with another data_name.

    augment (None, or an augment.Hyp / a dict / the path of a YAML file of one; `lod` and `coco`, either resize, either
    sensor): the reference's augment=True branch (dataset.py:483-514) without mosaic: per image the draws of
    augment.draw (random_perspective's affine matrix, augment_hsv's tables, the two flips), from a random.Random and a
    np.random.RandomState of their own, seeded from the source's seed and drawn on the calling thread in delivery order;
    the file order, the metadata draws and the noise keys of a seed stay what they are without it, and the batches are the
    same for every worker count. The descriptors and tables ride in the batch's one H2D copy and one adaisp_augment_u8
    launch (after adaisp_resize_u8 with resize="device") warps the letterboxed uint8 images, black around them as ever, into
    a device scratch of B frames of S x S; the unprocess / sensor kernels then read whole frames (h = w = S at (0, 0)).
    The labels go through augment.warp_labels; `paths` and `shapes` are unchanged. The warp comes BEFORE the sensor model
    (the reference warps the unprocessed, noisy float image, which smears white noise into correlated noise): the
    augmented S x S frame is the scene the sensor sees, so with add_noise or sensor="bayer" the black surround carries
    read noise and black level like any dark region, not the exact zeros of the un-augmented letterbox pad.
    With None nothing changes: no extra launch, no extra bytes, no extra draw. HIP devices only (RuntimeError on a CPU
    device); data_name="raw" raises ValueError (uint16 planes are not augmented).

    mosaic, mixup (probabilities, default 0; they need `augment`, and mixup needs mosaic > 0: ValueError otherwise, and for
    data_name="raw" or a value outside [0, 1]): the reference's `mosaic = random.random() < hyp['mosaic']` branch
    (dataset.py:822-830). Per delivered image, from the augmentation streams and where its index is handed out (so the
    partner images are decoded by the workers ahead of time like any other): random() < mosaic; if so augment.draw_mosaic
    (the centre, three more indices of this rank's files, the shuffle, random_perspective's draws), random() < mixup and if
    so randint(0, n - 1), a second draw_mosaic and the ratio beta(32, 32), then the HSV draw and the flips; if not, the
    whole augment.draw. A tile is load_image's output (the longer side at S; with resize="device" pass 1 of the resample
    alone). One adaisp_mosaic_u8 launch per batch samples the 2S x 2S canvases without building them and blends the mixed
    pairs; single images ride in the same launch as one-layer, one-tile records; the records travel in the batch's one H2D
    copy, which now carries up to 8 source images per output. The canvas and the border are black, this loader's letterbox
    colour. Labels: augment.mosaic_boxes per mosaic, concatenated for a mixup, augment.finish_labels. `paths` are those of
    the indices asked for, `shapes` of a mosaic is None. The sensor stages see B whole frames as after adaisp_augment_u8.
    With mosaic = 0 nothing changes: the same draws, the same adaisp_augment_u8 launch, the same bytes. Copy-paste is not
    built.

    On a CPU device `lod` is computed by torch exactly as LODImages does; `coco` and `raw` have no CPU path and raise."""

    def __init__(self, source, img_size, device, data_name="lod", add_noise=False, brightness_range=None, noise_level=None,
                 use_linear=False, seed=0, rank=0, world=1, workers=4, resize="host", sensor="rgb", cfa="RGGB", raw_bits=12,
                 black_level=None, demosaic="bilinear", raw_gains=(1.0, 1.0, 1.0), raw_calibration=None, raw_meta=False,
                 augment=None, mosaic=0.0, mixup=0.0):
        from ._lib import CFA, DEMOSAIC
        from .augment import Hyp
        from .rawcal import RawCalibration, read_sidecar, resolve
        if data_name not in ("lod", "coco", "raw"):
            raise ValueError(f"data_name must be 'lod', 'coco' or 'raw', got {data_name!r}")
        if resize not in ("host", "device"):
            raise ValueError(f"resize must be 'host' or 'device', got {resize!r}")
        if sensor not in ("rgb", "bayer"):
            raise ValueError(f"sensor must be 'rgb' or 'bayer', got {sensor!r}")
        if demosaic not in DEMOSAIC:
            raise ValueError(f"demosaic must be one of {sorted(DEMOSAIC)}, got {demosaic!r}")
        if not isinstance(cfa, str) or cfa.upper() not in CFA:
            raise ValueError(f"cfa must be one of {sorted(CFA)}, got {cfa!r}")
        if isinstance(raw_bits, bool) or not isinstance(raw_bits, (int, np.integer)) or not 1 <= raw_bits <= 16:
            raise ValueError(f"raw_bits must be an integer in [1, 16], got {raw_bits!r}")
        self.sensor, self.cfa, self.raw_bits, self.demosaic = sensor, cfa.upper(), int(raw_bits), demosaic
        self.white_level = 2 ** self.raw_bits - 1
        self.black_level = (2 ** (self.raw_bits - 6) if self.raw_bits >= 6 else 0) if black_level is None else black_level
        if not 0 <= self.black_level < self.white_level or int(self.black_level) != self.black_level:
            raise ValueError(f"black_level must be a whole number in [0, {self.white_level}), got {black_level!r}")
        self.black_level = int(self.black_level)
        self.device = torch.device(device)
        self.raw_gains = tuple(float(v) for v in raw_gains)
        if len(self.raw_gains) != 3 or not all(np.isfinite(self.raw_gains)):
            raise ValueError(f"raw_gains must be three finite numbers (R, G, B), got {raw_gains!r}")
        if data_name == "raw":
            if sensor == "bayer":
                raise ValueError("data_name='raw' with sensor='bayer': the plane already is a sensor's")
            if add_noise or brightness_range is not None or noise_level is not None or use_linear:
                raise ValueError("data_name='raw' takes the captures as they are: add_noise, brightness_range, noise_level "
                                 "and use_linear belong to data_name='coco'")
        self.augment = None if augment is None else Hyp(augment)
        for name, p in (("mosaic", mosaic), ("mixup", mixup)):
            if isinstance(p, bool) or not isinstance(p, (int, float, np.integer, np.floating)) or not 0 <= p <= 1:
                raise ValueError(f"{name} must be a probability in [0, 1], got {p!r}")
        self.mosaic, self.mixup = float(mosaic), float(mixup)
        if self.mosaic > 0 and self.augment is None:
            raise ValueError("mosaic needs augment (the mosaic is warped, coloured and flipped by its hyper-parameters)")
        if self.mosaic > 0 and data_name == "raw":
            raise ValueError("data_name='raw' with mosaic: uint16 planes are not augmented")
        if self.mixup > 0 and not self.mosaic > 0:
            raise ValueError("mixup needs mosaic > 0 (the reference mixes mosaics only)")
        if self.augment is not None and data_name == "raw":
            raise ValueError("data_name='raw' with augment: uint16 planes are not augmented")
        if self.augment is not None and self.device.type != "cuda":
            raise RuntimeError("ImageFolderSource(augment=...): the warp and the HSV tables run on the HIP device only "
                               "(adaisp_augment_u8); there is no CPU path")
        if data_name != "raw" and (raw_calibration is not None or raw_meta):
            raise ValueError("raw_calibration and raw_meta belong to data_name='raw'")
        if isinstance(raw_calibration, (str, os.PathLike)):
            raw_calibration = RawCalibration.load(raw_calibration)
        if raw_calibration is not None and not isinstance(raw_calibration, RawCalibration):
            raise ValueError(f"raw_calibration must be a RawCalibration or the path of one, got {type(raw_calibration).__name__}")
        if raw_calibration is not None and raw_calibration.cfa != self.cfa:
            raise ValueError(f"raw_calibration is of a {raw_calibration.cfa} sensor, cfa is {self.cfa}")
        self.raw_calibration, self.raw_meta = raw_calibration, bool(raw_meta)
        if sensor == "bayer" and self.device.type != "cuda":
            raise RuntimeError("ImageFolderSource(sensor='bayer'): the sensor and its demosaic run on the HIP device only "
                               "(adaisp_unprocess_bayer, adaisp_demosaic_rects_ex); there is no CPU path")
        if data_name == "coco" and self.device.type != "cuda":
            raise RuntimeError("ImageFolderSource(data_name='coco'): the unprocess runs on the HIP device only "
                               "(adaisp_unprocess); there is no CPU path")
        if resize == "device" and self.device.type != "cuda" and data_name != "raw":
            raise RuntimeError("ImageFolderSource(resize='device'): the resample runs on the HIP device only "
                               "(adaisp_resize_u8); there is no CPU path")
        self.resize = resize
        if add_noise and data_name != "coco":
            raise ValueError("add_noise needs data_name='coco'")
        if brightness_range is not None and isinstance(brightness_range, (list, tuple)):
            brightness_range = tuple(float(v) for v in brightness_range)
        if data_name == "raw":
            try:
                files = list_images(source, RAW_FORMATS)
            except FileNotFoundError:
                raise ValueError(f"{source}: data_name='raw' reads .npy planes and there is none") from None
        else:
            files = list_images(source)
        self.files = sorted(files)[rank::world]
        if not self.files:
            raise FileNotFoundError(f"{source}: no images for rank {rank} of {world}")
        if data_name == "raw":
            for f in self.files:
                open_raw_plane(f)                     # header only: a file that is no uint16 plane fails here, by name
            # sidecars are read here, once: a malformed one fails by name; levels that cannot be used fail by name too
            self._meta = {f: read_sidecar(f) for f in self.files} if self.raw_meta else {}
            for f in self.files:
                resolve(self.raw_calibration, self._meta.get(f), self.black_level, self.white_level,
                        where=f if self._meta.get(f) else "raw_calibration")
            self._rawfix = self.raw_calibration is not None or any(m is not None for m in self._meta.values())
            if self.device.type != "cuda":
                raise RuntimeError("ImageFolderSource(data_name='raw'): the demosaic and resample run on the HIP device only "
                                   "(adaisp_raw_load); there is no CPU path")
        self.img_size, self.data_name = int(img_size), data_name
        self.add_noise, self.brightness_range = bool(add_noise), brightness_range
        self.noise_level, self.use_linear = noise_level, bool(use_linear)
        self.seed = 1000 * int(seed) + int(rank)
        self.rng = random.Random(self.seed)
        self.rs = np.random.RandomState(self.seed)
        if self.augment is not None:              # streams of their own: self.rng / self.rs draw what they draw without
            self._aug_rng = random.Random(self.seed + AUGMENT_SEED)
            self._aug_rs = np.random.RandomState((self.seed + AUGMENT_SEED) % 2 ** 32)
        self.indices = list(range(len(self.files)))
        self.serial = 0
        self.workers = int(workers)
        self._pool = ThreadPoolExecutor(max_workers=self.workers) if self.workers > 0 else None
        self._ahead = deque()                     # (index, Future | decoded item), in delivery order
        self._slots = [dict(host=None, event=None) for _ in range(2)]
        self._slot = 0
        self._dev = None
        self._plane = None                        # sensor="bayer": the uint16 plane between the two kernels
        if data_name != "raw":
            self._meta, self._rawfix = {}, False

    def __len__(self):
        return len(self.files)

    def close(self):
        if self._pool is not None:
            self._pool.shutdown(wait=True, cancel_futures=True)
            self._pool = None

    def describe(self):
        if self.data_name == "raw":
            gains = "" if self.raw_gains == (1.0, 1.0, 1.0) else ", gains " + " ".join(f"{g:g}" for g in self.raw_gains)
            cal = "" if self.raw_calibration is None else f", calibration {self.raw_calibration.describe()}"
            if self.raw_meta:
                cal += f", {sum(m is not None for m in self._meta.values())} sidecars"
            return (f"raw ({self.cfa} {self.raw_bits}-bit black {self.black_level}, {self.demosaic} demosaic{gains}{cal}): "
                    f"{len(self.files)} files")
        kind = "coco (unprocess" + (", noise" if self.add_noise else "") + ")" if self.data_name == "coco" else "lod"
        bayer = f", bayer {self.cfa} {self.raw_bits}-bit black {self.black_level}" if self.sensor == "bayer" else ""
        if bayer and self.demosaic != "bilinear":
            bayer += f", {self.demosaic} demosaic"
        aug = "" if self.augment is None else f", augment ({self.augment.describe()})"
        if self.mosaic > 0:
            aug += f", mosaic {self.mosaic:g}" + (f", mixup {self.mixup:g}" if self.mixup > 0 else "")
        return f"{kind}: {len(self.files)} files" + (", device resize" if self.resize == "device" else "") + bayer + aug

    # ------------------------------------------------------------------------------------------------------ order
    def _next_index(self):
        i = self.indices[0]
        self.indices = self.indices[1:]
        if not self.indices:
            self.indices = list(range(len(self.files)))
            self.rng.shuffle(self.indices)
        return i

    def _decode(self, i, tile=False):
        """File i as an Item (which says what its fields hold in each mode); `tile`: as a mosaic tile."""
        path = self.files[i]
        if tile:
            if self.resize != "device":
                im, size = np.ascontiguousarray(load_image(path, self.img_size, augment=False)[0]), None
            else:
                im = imread_bgr(path)
                size = letterboxed_geometry(im.shape[0], im.shape[1], self.img_size)[0]
            return Item(im, 0, 0, np.zeros((0, 6), np.float32), path, None, size, size, read_labels(_label_path(path)))
        if self.data_name != "raw" and self.resize != "device":
            im, (top, left), _, lb, shapes = load_letterboxed(path, self.img_size)
            size = unpad = None
        else:
            im = open_raw_plane(path) if self.data_name == "raw" else imread_bgr(path)
            size, unpad, (top, left), frame, ratio, pad, shapes = letterboxed_geometry(im.shape[0], im.shape[1], self.img_size)
            lb = letterboxed_labels(path, size, frame, ratio, pad)
        return Item(im, top, left, _label6(lb), path, shapes, size, unpad)

    def _next_sample(self):
        """mosaic > 0: the next index and the draws of its image (the class docstring's order). Returns (SamplePlan,
        [(file index, as a tile?)] to decode)."""
        from .augment import Draw, draw, draw_colour_flips, draw_mosaic
        hyp, rng, nprs, S, n = self.augment, self._aug_rng, self._aug_rs, self.img_size, len(self.files)
        i = self._next_index()
        if not rng.random() < self.mosaic:
            return SamplePlan(i, (), None, draw(hyp, rng, nprs, S)), [(i, False)]
        mosaics, r = (draw_mosaic(hyp, rng, nprs, S, n, i),), None
        if rng.random() < self.mixup:
            mosaics += (draw_mosaic(hyp, rng, nprs, S, n, rng.randint(0, n - 1)),)
            r = float(nprs.beta(32.0, 32.0))
        luts, flipud, fliplr = draw_colour_flips(hyp, rng, nprs)
        return (SamplePlan(i, mosaics, r, Draw(mosaics[0].M, mosaics[0].s, flipud, fliplr, luts)),
                [(k, True) for mz in mosaics for k in mz.indices])

    def _take_samples(self, n):
        """mosaic > 0: the next n Samples; with workers, keeps up to 2 * n more decoding behind them."""
        if self._pool is None:
            out = []
            for _ in range(n):
                plan, jobs = self._next_sample()
                out.append(Sample(plan, [self._decode(k, tile) for k, tile in jobs]))
            return out
        while len(self._ahead) < 2 * n:
            plan, jobs = self._next_sample()
            self._ahead.append((plan, [self._pool.submit(self._decode, k, tile) for k, tile in jobs]))
        taken = [self._ahead.popleft() for _ in range(n)]
        return [Sample(plan, [f.result() for f in futures]) for plan, futures in taken]

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
        if self.mosaic > 0:
            samples = self._take_samples(n)
            plan = self._mosaic_plan(samples)
            paths = [self.files[s.plan.index] for s in samples]
            shapes = [None if s.plan.mosaics else s.items[0].shapes for s in samples]
            return list(self._device_batch(plan["items"], plan)), plan["labels"], paths, shapes
        items = self._take(n)
        labels, paths, shapes = [it.label for it in items], [it.path for it in items], [it.shapes for it in items]
        if self.device.type != "cuda":
            return list(self._cpu_lod(items)), labels, paths, shapes
        plan = None
        if self.augment is not None:
            plan = self._augment_plan(items)
            labels = plan["labels"]
        return list(self._device_batch(items, plan)), labels, paths, shapes

    def _augment_plan(self, items):
        """The host half of a batch's augmentation, no device: per item, in delivery order, augment.draw from the source's
        two augmentation streams. Returns dict(m: int64 [B,6], the Q16 inverse maps with the flips folded in; lut: int32
        [B], each image's table or -1; luts: uint8 [n,768]; labels: the warped [k,6] float32 rows; draws: the Draws;
        records: AUGMENT_DESC [B], all but src_offset, which the staging decides; slots: (image, position in items))."""
        from . import _lib
        from .augment import draw, fixed_inverse, warp_labels
        S, B = self.img_size, len(items)
        rec = np.zeros(B, _lib.AUGMENT_DESC)
        luts, labels, draws = [], [], []
        for b, it in enumerate(items):
            d = draw(self.augment, self._aug_rng, self._aug_rs, S)
            rec[b]["h"], rec[b]["w"] = it.pixels.shape[:2] if it.unpad is None else it.unpad
            rec[b]["top"], rec[b]["left"], rec[b]["lut"] = it.top, it.left, _table_index(luts, d)
            rec[b]["m"] = fixed_inverse(d.M, d.flipud, d.fliplr, S)
            labels.append(_label6(warp_labels(it.label[:, 1:], d.M, d.s, d.flipud, d.fliplr, S)))
            draws.append(d)
        luts = np.stack(luts) if luts else np.zeros((0, 768), np.uint8)
        return dict(m=rec["m"].copy(), lut=rec["lut"].copy(), luts=luts, labels=labels, draws=draws, records=rec,
                    slots=[(b, b) for b in range(B)])

    def _mosaic_plan(self, samples):
        """The host half of a batch of a source with mosaic > 0, no device: the adaisp_mosaic_u8 records of the Samples (all
        but the tiles' src_offset, which the staging decides), their tables and labels. Returns dict(records: MOSAIC_DESC
        [B]; n_layers: the launch's; lut: int32 [B]; luts: uint8 [n,768]; labels: the [k,6] float32 rows; items: the Items
        to stage, flat; slots: (image, layer, tile, position in items) of every tile; plans: the SamplePlans)."""
        from . import _lib
        from .augment import (fill_mosaic_layer, fill_single_layer, finish_labels, fixed_inverse, mix_q16, mosaic_boxes,
                              mosaic_tiles, warp_labels)
        S, B = self.img_size, len(samples)
        rec = np.zeros(B, _lib.MOSAIC_DESC)
        rec["n_layers"], rec["mix"] = 1, _lib.MOSAIC_MIX_ONE
        luts, labels, items, slots = [], [], [], []
        for b, (plan, its) in enumerate(samples):
            d = plan.draw
            rec[b]["lut"] = _table_index(luts, d)
            if not plan.mosaics:                  # a single image is one layer with one tile
                it = its[0]
                h, w = it.pixels.shape[:2] if it.unpad is None else it.unpad
                fill_single_layer(rec[b]["layer"][0], fixed_inverse(d.M, d.flipud, d.fliplr, S), h, w, it.top, it.left)
                rows = warp_labels(it.label[:, 1:], d.M, d.s, d.flipud, d.fliplr, S)
            else:
                rec[b]["n_layers"] = len(plan.mosaics)
                if plan.r is not None:
                    rec[b]["mix"] = mix_q16(plan.r)
                boxes = []
                for l, mz in enumerate(plan.mosaics):
                    four = its[4 * l:4 * l + 4]
                    sizes = [tuple(it.pixels.shape[:2]) if it.size is None else tuple(it.size) for it in four]
                    tiles = mosaic_tiles(sizes, mz.centre, S)
                    fill_mosaic_layer(rec[b]["layer"][l], fixed_inverse(mz.M, d.flipud, d.fliplr, S), sizes, tiles)
                    boxes.append(mosaic_boxes([it.native for it in four], sizes, tiles, mz.M, mz.s, S))
                rows = finish_labels(np.concatenate(boxes), S, d.flipud, d.fliplr)
            for k, it in enumerate(its):          # the Items are the tiles, layer by layer
                slots.append((b, k // 4, k % 4, len(items)))
                items.append(it)
            labels.append(_label6(rows))
        luts = np.stack(luts) if luts else np.zeros((0, 768), np.uint8)
        return dict(records=rec, n_layers=int(rec["n_layers"].max()), lut=rec["lut"].copy(), luts=luts, labels=labels,
                    items=items, slots=slots, plans=[s.plan for s in samples])

    def _cpu_lod(self, items):
        S = self.img_size
        out = torch.zeros((len(items), 3, S, S))
        for b, it in enumerate(items):
            h, w = it.pixels.shape[:2]
            chw = np.ascontiguousarray(it.pixels.transpose(2, 0, 1)[::-1])
            out[b, :, it.top:it.top + h, it.left:it.left + w] = torch.from_numpy(chw).float() / 255.0
        return out.to(self.device)

    def _resize_plan(self, items, head):
        """Device resize: the byte layout after the unprocess descriptors (`head` bytes) and the two adaisp_resize_u8
        calls. Staged (one H2D copy): descriptors of pass 1 / pass 2, their tap tables, the decoded images; after them,
        device only: scratch 1 (load_image's resample of the images with r != 1) and scratch 2 (letterbox's resample of
        the ceil overshoots, from scratch 1). Returns (layout dict, [(h, w, offset) of every final image relative to the
        first decoded image])."""
        from .resize import TapPlan
        S = self.img_size
        p1 = TapPlan()
        sizes, pix = [], 0
        for it in items:
            sizes.append((it.pixels.shape[:2], pix, it.size, it.unpad))
            pix += it.pixels.size
        off1, at1 = 0, {}
        for b, (full, src_off, size, _unpad) in enumerate(sizes):
            if tuple(size) != tuple(full):
                p1.add(full, size, max(full) > S, src_off, off1)
                at1[b] = off1
                off1 += size[0] * size[1] * 3
        p2 = TapPlan(base=p1.words)
        off2, final = 0, []
        for b, (full, src_off, size, unpad) in enumerate(sizes):
            if tuple(unpad) != tuple(size):
                p2.add(size, unpad, False, at1[b], off2)
                final.append((unpad[0], unpad[1], pix + off1 + off2))
                off2 += unpad[0] * unpad[1] * 3
            elif b in at1:
                final.append((size[0], size[1], pix + at1[b]))
            else:
                final.append((full[0], full[1], src_off))
        rec1, rec2 = p1.descriptors(), p2.descriptors()
        tab = np.concatenate([p1.table(), p2.table()])
        r1, r2, tb, base = _sections(head, rec1.nbytes, rec2.nbytes, tab.nbytes)
        lay = dict(rec1=rec1, rec2=rec2, tab=tab, r1=r1, r2=r2, tb=tb, base=base, s1=off1, s2=off2)
        return lay, final

    def _stage(self, total, fill, scratch=0, room=0):
        """What every batch does with its bytes: the next pinned slot, once the event of its previous copy has completed;
        host and device buffers grown to `total` bytes (the host at least to `room`, the device by `scratch` more, which
        only kernels write); `fill(host)` writes the first `total` bytes of the slot (a numpy view); the batch's one H2D
        copy, non-blocking on the current stream, and the slot's event behind it. Returns the device buffer."""
        slot = self._slots[self._slot]
        self._slot = (self._slot + 1) % len(self._slots)
        if slot["event"] is not None:
            slot["event"].synchronize()           # this slot's previous H2D copy has finished reading it
        if slot["host"] is None or slot["host"].numel() < total:
            slot["host"] = torch.empty(max(total, room), dtype=torch.uint8, pin_memory=True)
        fill(slot["host"].numpy())
        if self._dev is None or self._dev.numel() < total + scratch:
            self._dev = torch.empty(max(slot["host"].numel(), total + scratch), dtype=torch.uint8, device=self.device)
        self._dev[:total].copy_(slot["host"][:total], non_blocking=True)
        slot["event"] = torch.cuda.Event()
        slot["event"].record()
        return self._dev

    def _raw_batch(self, items):
        """data_name="raw": one pinned buffer (descriptors, tap tables, the planes, each 16-byte aligned), one H2D copy, one
        adaisp_raw_load on the current stream. With a calibration or sidecars in play the adaisp_raw_correct descriptors
        and the shading table ride in the same buffer between the tap tables and the planes, the device buffer has a
        second plane region behind the first, adaisp_raw_correct runs from the first into the second (every capture with
        its own levels, brought to the run's black and white level) and adaisp_raw_load reads the second."""
        from . import _lib
        from .rawcal import fill_rawfix, level_scale, resolve
        from .resize import RawTapPlan
        S, B = self.img_size, len(items)
        *at, pos = _sections(0, *(it.pixels.nbytes for it in items))          # the planes, relative to the first
        plan = RawTapPlan()
        for it, off in zip(items, at):
            if min(it.pixels.shape) < 2:
                raise ValueError(f"{it.path}: {it.pixels.shape[0]} x {it.pixels.shape[1]} samples: a raw plane needs at least "
                                 "2 x 2")
            meta = self._meta.get(it.path) or {}
            plan.add(it.pixels.shape, it.unpad, (it.top, it.left), off, meta.get("gains", self.raw_gains))
        self.serial += B
        desc, tab = plan.descriptors(), plan.table()
        _, dbytes, base = _sections(0, desc.nbytes, tab.nbytes)
        fix = shading = None
        if self._rawfix:
            cal = self.raw_calibration
            shading = None if cal is None else cal.shading
            fix = np.zeros(B, _lib.RAWFIX_DESC)
            for k, it in enumerate(items):
                black, white = resolve(cal, self._meta.get(it.path), self.black_level, self.white_level, where=it.path)
                fill_rawfix(fix[k], it.pixels.shape, at[k], at[k], black,
                            level_scale(black, white, self.black_level, self.white_level), self.black_level,
                            None if cal is None else cal.dpc, None if shading is None else (0, *shading.shape[1:]))
            fbase, gbase, base = _sections(base, fix.nbytes, 0 if shading is None else shading.nbytes)
        total = base + pos

        def fill(host):
            host[:desc.nbytes] = desc.view(np.uint8)
            host[dbytes:dbytes + tab.nbytes] = tab.view(np.uint8)
            if fix is not None:
                host[fbase:fbase + fix.nbytes] = fix.view(np.uint8)
                if shading is not None:
                    host[gbase:gbase + shading.nbytes] = shading.reshape(-1).view(np.uint8)

            def copy(k):                          # the one host pass over the samples: mapping -> pinned slot
                plane = items[k].pixels
                host[base + at[k]:base + at[k] + plane.nbytes].view(np.uint16).reshape(plane.shape)[...] = plane

            if self._pool is not None:
                list(self._pool.map(copy, range(B)))
            else:
                for k in range(B):
                    copy(k)

        with torch.cuda.device(self.device):
            dev = self._stage(total, fill, scratch=pos if fix is not None else 0)
            planes = dev[base:total]
            if fix is not None:
                gains = None if shading is None else dev[gbase:gbase + shading.nbytes].view(torch.float32)
                planes = _lib.raw_correct(planes, dev[fbase:fbase + fix.nbytes], gains, out=dev[total:total + pos])
            return _lib.raw_load(planes, dev[:desc.nbytes], dev[dbytes:dbytes + tab.nbytes], S, pattern=self.cfa,
                                 method=self.demosaic, black_level=self.black_level, white_level=self.white_level)

    def _device_batch(self, items, plan=None):
        """`plan` (of _augment_plan or _mosaic_plan): the batch is augmented: the plan's records, their source offsets
        patched in, and its tables are staged behind the unprocess descriptors, adaisp_augment_u8 (AUGMENT_DESC records) or
        adaisp_mosaic_u8 (MOSAIC_DESC: `items` are then the sources to stage, several per frame) writes B whole frames
        into device scratch behind everything else, and the unprocess descriptors describe those frames."""
        from . import _lib
        if self.data_name == "raw":
            return self._raw_batch(items)
        S, B = self.img_size, len(items) if plan is None else len(plan["lut"])
        desc = np.zeros(B, _lib.UNPROCESS_DESC)
        if plan is None:
            _, dbytes = _sections(0, desc.nbytes)
        else:
            adesc, luts = plan["records"], plan["luts"]
            _, a_at, l_at, dbytes = _sections(0, desc.nbytes, adesc.nbytes, luts.nbytes)
        lay = None
        if self.resize == "device":
            lay, final = self._resize_plan(items, dbytes)
        else:
            final, off = [], 0
            for it in items:
                final.append((it.pixels.shape[0], it.pixels.shape[1], off))
                off += it.pixels.size
        if plan is not None:
            where = (adesc if adesc.dtype == _lib.AUGMENT_DESC else adesc["layer"]["tile"])["src_offset"]      # a view
            for *at, k in plan["slots"]:
                where[tuple(at)] = final[k][2]
        for b in range(B):
            if plan is None:
                (h, w, src_offset), top, left = final[b], items[b].top, items[b].left
            else:                                 # the images go to the warp; the sensor sees the whole warped frames
                h, w, src_offset, top, left = S, S, b * S * S * 3, 0, 0
            if self.sensor == "bayer" and min(h, w) < 2:
                raise ValueError(f"{items[b].path}: {h} x {w} pixels at size {S}: sensor='bayer' needs at least 2 x 2")
            desc[b]["src_offset"], desc[b]["h"], desc[b]["w"] = src_offset, h, w
            desc[b]["top"], desc[b]["left"], desc[b]["serial"] = top, left, self.serial
            self.serial += 1
        flags = 0
        if self.data_name == "coco":
            flags = _lib.UNP_UNPROCESS | (_lib.UNP_NOISE if self.add_noise else 0)
            for b in range(B):
                desc[b]["p"] = kernel_params(sample_unprocess_params(self.rs, self.add_noise, self.brightness_range,
                                                                     self.noise_level, self.use_linear))
        base = dbytes if lay is None else lay["base"]                   # where the staged pixels start
        total = base + sum(it.pixels.size for it in items)
        need = total if lay is None else total + lay["s1"] + lay["s2"]
        frames = (need + 15) // 16 * 16                                 # augmented: B whole frames, device only
        end = need if plan is None else frames + B * S * S * 3

        def fill(host):
            host[:desc.nbytes] = desc.view(np.uint8)
            if plan is not None:
                host[a_at:a_at + adesc.nbytes] = adesc.view(np.uint8)
                host[l_at:l_at + luts.nbytes] = luts.reshape(-1)
            if lay is not None:
                for key, at in (("rec1", "r1"), ("rec2", "r2"), ("tab", "tb")):
                    host[lay[at]:lay[at] + lay[key].nbytes] = lay[key].view(np.uint8)
            pos = base
            for it in items:
                host[pos:pos + it.pixels.size] = it.pixels.reshape(-1)
                pos += it.pixels.size

        with torch.cuda.device(self.device):
            dev = self._stage(total, fill, scratch=end - total, room=dbytes + B * S * S * 3)
            if lay is not None:
                self._resize_on_device(lay, total)
            pixels, records = dev[base:need], dev[:desc.nbytes]
            if plan is not None:                  # the fills are 0 either way: the canvas and the border are black
                args = pixels, dev[a_at:a_at + adesc.nbytes], dev[l_at:l_at + luts.nbytes] if luts.size else None, S
                if adesc.dtype == _lib.AUGMENT_DESC:
                    pixels = _lib.augment_u8(*args, fill=0, out=dev[frames:end], records=adesc)
                else:
                    pixels = _lib.mosaic_u8(*args, n_layers=plan["n_layers"], out=dev[frames:end], records=adesc)
            if self.sensor != "bayer":
                return _lib.unprocess(pixels, records, S, seed=self.seed, flags=flags)
            if self._plane is None or self._plane.shape[0] < B:
                self._plane = torch.empty((B, S, S), dtype=torch.uint16, device=self.device)
            levels = dict(pattern=self.cfa, black_level=self.black_level, white_level=self.white_level)
            raw = _lib.unprocess_bayer(pixels, records, S, seed=self.seed, flags=flags, out=self._plane[:B], **levels)
            return _lib.demosaic_rects(raw, records, method=self.demosaic, **levels)

    def _resize_on_device(self, lay, total):
        """The two adaisp_resize_u8 calls of a staged batch (see _resize_plan), on the current stream."""
        from . import _lib
        dev, s1, s2 = self._dev, lay["s1"], lay["s2"]
        tabs = dev[lay["tb"]:lay["tb"] + lay["tab"].nbytes] if lay["tab"].size else None
        if len(lay["rec1"]):
            _lib.resize_u8(dev[lay["base"]:total], dev[total:total + s1], dev[lay["r1"]:lay["r1"] + lay["rec1"].nbytes],
                           tabs, lay["rec1"])
        if len(lay["rec2"]):
            _lib.resize_u8(dev[total:total + s1], dev[total + s1:total + s1 + s2],
                           dev[lay["r2"]:lay["r2"] + lay["rec2"].nbytes], tabs, lay["rec2"])
