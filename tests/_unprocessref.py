"""Float64 numpy restatement of the unprocess chain (isp/unprocess_np.py:53-80,131-181; what adaisp_unprocess computes in
fp32), pinned to tests/golden/unprocess.npz by tests/test_unprocess_host.py and used by the GPU tests at any shape; and a
restatement of the kernel's noise generator (Philox4x32-10 + Box-Muller) for a few pixels."""
import numpy as np


def unprocess_clean(bgr_u8, rgb2cam, rgb_gain, red_gain, blue_gain, prescale=0.9, ratio=1.0):
    """uint8 HWC BGR -> float64 HWC RGB: unprocess_wo_mosaic without noise (the mask and clips included)."""
    x = np.clip(bgr_u8[..., ::-1] / 255.0 * prescale, 0.0, 1.0)
    x = 0.5 - np.sin(np.arcsin(1.0 - 2.0 * x) / 3.0)
    x = np.maximum(x, 1e-8) ** 2.2
    x = x @ np.asarray(rgb2cam, np.float64).T
    gains = np.array([1.0 / red_gain, 1.0, 1.0 / blue_gain]) / rgb_gain
    gray = np.mean(x, axis=-1, keepdims=True)
    mask = (np.maximum(gray - 0.9, 0.0) / (1.0 - 0.9)) ** 2.0
    x = x * np.maximum(mask + (1.0 - mask) * gains, gains)
    return np.clip(x, 0.0, 1.0) * ratio


def saturation_mask(bgr_u8, rgb2cam, prescale=1.0):
    """safe_invert_gains' mask per pixel (to check that a case reaches it)."""
    x = np.clip(bgr_u8[..., ::-1] / 255.0 * prescale, 0.0, 1.0)
    x = np.maximum(0.5 - np.sin(np.arcsin(1.0 - 2.0 * x) / 3.0), 1e-8) ** 2.2 @ np.asarray(rgb2cam, np.float64).T
    return (np.maximum(x.mean(-1) - 0.9, 0.0) / (1.0 - 0.9)) ** 2.0


def letterboxed(img_hwc, S, top, left):
    """An HWC result placed in a zero [3,S,S] frame."""
    out = np.zeros((3, S, S), img_hwc.dtype)
    h, w = img_hwc.shape[:2]
    out[:, top:top + h, left:left + w] = img_hwc.transpose(2, 0, 1)
    return out


M = 0xFFFFFFFF


def philox4x32_10(ctr, key):
    """Random123's philox4x32 with 10 rounds; ctr: 4 uint32, key: 2 uint32 -> 4 uint32."""
    c0, c1, c2, c3 = (int(v) & M for v in ctr)
    k0, k1 = (int(v) & M for v in key)
    for _ in range(10):
        p0, p1 = 0xD2511F53 * c0, 0xCD9E8D57 * c2
        c0, c1, c2, c3 = ((p1 >> 32) ^ c1 ^ k0) & M, p1 & M, ((p0 >> 32) ^ c3 ^ k1) & M, p0 & M
        k0, k1 = (k0 + 0x9E3779B9) & M, (k1 + 0xBB67AE85) & M
    return c0, c1, c2, c3


def normals3(seed, serial, idx):
    """The three N(0, 1) draws of pixel `idx` (index in the un-padded image) of image (seed, serial), float64."""
    r = philox4x32_10((idx, serial >> 32, seed >> 32, 0), (seed & M, serial & M))
    u1 = lambda v: ((v >> 8) + 1) * 2.0 ** -24          # noqa: E731  (0, 1]
    u2 = lambda v: (v >> 8) * 2.0 ** -24                # noqa: E731  [0, 1)
    r0, r1 = np.sqrt(-2.0 * np.log(u1(r[0]))), np.sqrt(-2.0 * np.log(u1(r[2])))
    return np.array([r0 * np.cos(2 * np.pi * u2(r[1])), r0 * np.sin(2 * np.pi * u2(r[1])), r1 * np.cos(2 * np.pi * u2(r[3]))])


def write_dataset(root, sizes, seed=0, unlabeled=(1,), nc=80):
    """A toy YOLO dataset under root/images + root/labels, written by PIL: image i has size sizes[i] = (h, w), PNG for
    even i and JPEG for odd i; images listed in `unlabeled` have no label file. Returns the image paths in sorted order."""
    import os
    from PIL import Image
    rs = np.random.RandomState(seed)
    os.makedirs(os.path.join(root, "images"), exist_ok=True)
    os.makedirs(os.path.join(root, "labels"), exist_ok=True)
    paths = []
    for i, (h, w) in enumerate(sizes):
        im = rs.randint(0, 256, size=(h, w, 3)).astype(np.uint8)
        im[0, 0] = 0
        im[-1, -1] = 255
        p = os.path.join(root, "images", f"im{i:03d}." + ("png" if i % 2 == 0 else "jpg"))
        Image.fromarray(im).save(p, **({"quality": 90} if i % 2 else {}))
        paths.append(p)
        if i not in unlabeled:
            k = 1 + i % 3
            with open(os.path.join(root, "labels", f"im{i:03d}.txt"), "w") as f:
                for _ in range(k):
                    cx, cy = rs.uniform(0.2, 0.8, 2)
                    bw, bh = rs.uniform(0.05, 0.3, 2)
                    f.write(f"{rs.randint(nc)} {cx:.6f} {cy:.6f} {bw:.6f} {bh:.6f}\n")
    return sorted(paths)
