#!/usr/bin/env python3
"""Fixture generator for the mosaic / mixup augmentation: imports the REFERENCE's utils/dataloaders.py, utils/augmentations.py
and utils/general.py unmodified (the stubs and the cv2 stand-in of gen_augment.py) and records, per case, what
`LoadImagesAndLabels.load_mosaic` makes of seeded draws, seeded uint8 tiles and their label sets: tests/golden/mosaic_aug.npz
(mosaic.npz is the Bayer sensor's fixture, of gen_golden.py).
`load_mosaic` runs on a stand-in `self` (img_size, mosaic_border, indices, labels, empty segments, hyp with copy_paste 0 and
a load_image that returns the seeded tiles); the reference's own slicing builds the 2S x 2S canvas, and the stand-in
`warpAffine` records that canvas and the matrix it is given. The mixup cases record the ratio and the reference's `mixup` of
two seeded uint8 frames and two of the recorded label sets.

Runs only where the reference is checked out (no GPU needed); the fixture it writes is committed next to it.

    python tests/golden/gen_mosaic.py [--out DIR]
"""
import os
import random
import sys
import types

import numpy as np

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from gen_augment import KEYS, LOW, STRONG, import_reference  # noqa: E402

BOXES = [[3, 0.50, 0.50, 0.30, 0.20], [7, 0.25, 0.30, 0.10, 0.40], [0, 0.70, 0.75, 0.20, 0.20]]
LEAVING = [[6, 0.04, 0.05, 0.16, 0.12], [8, 0.97, 0.95, 0.20, 0.22], [9, 0.50, 0.02, 0.30, 0.10], [2, 0.5, 0.5, 0.9, 0.9]]
REJECTED = [[1, 0.50, 0.50, 0.004, 0.30],      # under 2 px wide after the warp
            [4, 0.50, 0.50, 0.90, 0.004],      # under 2 px high
            [5, 0.50, 0.50, 0.25, 0.25]]       # kept where its tile is


def tile_sizes(kind, S):
    """Six (h, w) per kind. load_image brings the longer side to S; smaller ones stand for images it leaves alone."""
    q, h, t = S // 4, S // 2, 3 * S // 4
    return {"small": [(q, q + 3), (q + 5, q), (h - 3, q), (q, h - 1), (q + 1, q + 1), (5, 7)],
            "large": [(S, S)] * 6,
            "mixed": [(S, 5 * S // 8), (t, S), (S, S), (S, h + 1), (h - 1, S), (S, t)],
            }[kind]


# (name, S, seed, hyp, tile sizes of the n images, label rows of every image, the index asked for)
CASES = []
for S in (32, 64):
    CASES.append((f"small_{S}", S, 50, STRONG, tile_sizes("small", S), [BOXES] * 6, 2))
    CASES.append((f"large_{S}", S, 51, LOW, tile_sizes("large", S), [BOXES] * 6, 0))
    CASES.append((f"mixed_{S}", S, 52, STRONG, tile_sizes("mixed", S), [BOXES, LEAVING, [], BOXES[:1], LEAVING, BOXES], 5))
    CASES.append((f"empty_{S}", S, 53, STRONG, tile_sizes("mixed", S), [[]] * 6, 1))
    CASES.append((f"leaving_{S}", S, 54, dict(LOW, translate=0.3, scale=0.1), tile_sizes("large", S), [LEAVING] * 6, 3))
    CASES.append((f"rejected_{S}", S, 55, dict(LOW, scale=0.05, translate=0.0), tile_sizes("mixed", S), [REJECTED] * 6, 4))
# (name, S, seed, the two cases whose labels are concatenated)
MIXUPS = [(f"mixup_{S}_{k}", S, 60 + k, f"mixed_{S}", f"small_{S}") for S in (32, 64) for k in range(2)]


def tiles_of(seed, sizes):
    """The seeded uint8 tiles of a case (the tests rebuild them from the recorded seed and sizes)."""
    rs = np.random.RandomState(seed)
    return [rs.randint(0, 256, size=(h, w, 3)).astype(np.uint8) for h, w in sizes]


def main(out_dir=HERE):
    cv2, A, G = import_reference()
    from utils import dataloaders as D
    seen = {}

    def warp_affine(im, M, dsize, borderValue=None):
        seen["canvas"], seen["M"] = np.array(im), np.array(M, np.float64)
        return np.zeros((dsize[1], dsize[0], 3), im.dtype)

    cv2.warpAffine = warp_affine
    out = {"names": np.frombuffer("\n".join([c[0] for c in CASES] + [c[0] for c in MIXUPS]).encode(), np.uint8)}
    kept = {}
    for name, S, seed, hyp, sizes, rows, index in CASES:
        tiles = tiles_of(seed, sizes)
        labels = [np.array(r, np.float64).reshape(-1, 5) for r in rows]
        order = []

        def load_image(i, tiles=tiles, order=order):
            order.append(i)
            return tiles[i], None, tiles[i].shape[:2]

        me = types.SimpleNamespace(img_size=S, mosaic_border=[-S // 2, -S // 2], indices=range(len(tiles)), labels=labels,
                                   segments=[[] for _ in tiles], hyp=dict(hyp, copy_paste=0.0), load_image=load_image)
        # the centre is the first two draws, the scale the fourth uniform of random_perspective's eight behind choices and
        # shuffle: read them back from a twin generator
        twin = random.Random(seed)
        yc, xc = (int(twin.uniform(-x, 2 * S + x)) for x in me.mosaic_border)
        picks = [index] + twin.choices(range(len(tiles)), k=3)
        twin.shuffle(picks)
        for _ in range(3):
            twin.uniform(0, 1)
        s = twin.uniform(1 - hyp["scale"], 1 + hyp["scale"])
        random.seed(seed)
        np.random.seed(seed)
        seen.clear()
        _, warped = D.LoadImagesAndLabels.load_mosaic(me, index)
        assert order == picks and seen["canvas"].shape == (2 * S, 2 * S, 3)
        M = np.eye(3)
        M[:2] = seen["M"]
        warped = np.array(warped, np.float64).reshape(-1, 5)
        final = warped.copy()
        if len(final):
            final[:, 1:5] = G.xyxy2xywhn(final[:, 1:5], w=S, h=S, clip=True, eps=1E-3)
        kept[name] = warped
        out[f"{name}/S"], out[f"{name}/seed"], out[f"{name}/index"] = np.int64(S), np.int64(seed), np.int64(index)
        out[f"{name}/hyp_values"] = np.array([hyp[k] for k in KEYS], np.float64)
        out[f"{name}/sizes"] = np.array(sizes, np.int64)
        out[f"{name}/labels_in"] = np.concatenate([np.concatenate([np.full((len(lb), 1), i, np.float64), lb], 1)
                                                   for i, lb in enumerate(labels)])            # image, class, x y w h
        out[f"{name}/centre"], out[f"{name}/order"] = np.array([xc, yc], np.int64), np.array(order, np.int64)
        out[f"{name}/canvas"], out[f"{name}/M"], out[f"{name}/s"] = seen["canvas"], M, np.float64(s)
        out[f"{name}/labels_warped"], out[f"{name}/labels_out"] = warped, final
        print(f"{name}: centre ({xc}, {yc}), order {order}, s = {s:.4f}, {sum(map(len, labels))} rows in the set, "
              f"{sum(len(labels[i]) for i in order)} placed -> {len(final)} labels")
    for name, S, seed, first, second in MIXUPS:
        rs = np.random.RandomState(seed)
        a, b = (rs.randint(0, 256, size=(S, S, 3)).astype(np.uint8) for _ in range(2))
        np.random.seed(seed)
        r = np.random.RandomState(seed).beta(32.0, 32.0)
        im, labels = A.mixup(a, kept[first], b, kept[second])
        final = np.array(labels, np.float64)
        final[:, 1:5] = G.xyxy2xywhn(final[:, 1:5], w=S, h=S, clip=True, eps=1E-3)
        out[f"{name}/S"], out[f"{name}/seed"], out[f"{name}/r"] = np.int64(S), np.int64(seed), np.float64(r)
        out[f"{name}/mixed"], out[f"{name}/labels_out"] = np.array(im, np.uint8), final
        out[f"{name}/of"] = np.frombuffer(f"{first}\n{second}".encode(), np.uint8)
        print(f"{name}: r = {r:.6f}, {len(final)} labels")
    path = os.path.join(out_dir, "mosaic_aug.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main(sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else HERE)
