"""numpy int64 restatement of adaisp_mosaic_u8, written from the header comment (include/adaisp.h, csrc/isp_augment.hip):
per layer the fixed-point affine warp of a canvas made of up to four tiles, the Q16 blend of two layers, then
_augref.colour's table chain. It calls no package code: a record is anything indexed by the field names of
adaisp_mosaic_desc (a numpy record, or nested dicts and lists)."""
import numpy as np

from _augref import colour, fill_triple


def tile_present(t, src_bytes):
    h, w = int(t["h"]), int(t["w"])
    x0, y0, x1, y1, dx, dy = (int(t[k]) for k in ("x0", "y0", "x1", "y1", "dx", "dy"))
    off = int(t["src_offset"])
    return (0 <= h <= 32768 and 0 <= w <= 32768 and x0 <= x1 and y0 <= y1 and x0 - dx >= 0 and x1 - dx <= w and y0 - dy >= 0
            and y1 - dy <= h and off >= 0 and off + h * w * 3 <= src_bytes)


def layer(src, L, S):
    """One layer's v for every output pixel: int64 [S,S,3]. `src`: the uint8 bytes the tiles' offsets point into."""
    src = np.asarray(src, np.uint8).reshape(-1)
    m = [np.int64(v) for v in np.asarray(L["m"]).tolist()]
    x = np.arange(S, dtype=np.int64)[None, :]
    y = np.arange(S, dtype=np.int64)[:, None]
    with np.errstate(over="ignore"):
        fx = m[0] * x + m[1] * y + m[2]
        fy = m[3] * x + m[4] * y + m[5]
    X, Y = fx >> 16, fy >> 16
    ax, ay = ((fx >> 11) & 31)[..., None], ((fy >> 11) & 31)[..., None]
    pad = np.array(fill_triple(int(L["fill"])), np.int64)
    n = min(max(int(L["n_tiles"]), 0), 4)
    tiles = [L["tile"][t] for t in range(n) if tile_present(L["tile"][t], src.size)]
    padded = np.concatenate([src.astype(np.int64), np.zeros(3, np.int64)])

    def P(i, j):
        out = np.broadcast_to(pad, i.shape + (3,)).copy()
        taken = np.zeros(i.shape, bool)
        for t in tiles:
            inside = (i >= int(t["x0"])) & (i < int(t["x1"])) & (j >= int(t["y0"])) & (j < int(t["y1"])) & ~taken
            at = np.where(inside, int(t["src_offset"]) + ((j - int(t["dy"])) * int(t["w"]) + (i - int(t["dx"]))) * 3, src.size)
            px = np.stack([padded[at], padded[np.minimum(at + 1, src.size)], padded[np.minimum(at + 2, src.size)]], -1)
            out = np.where(inside[..., None], px, out)
            taken |= inside
        return out

    return ((32 - ax) * (32 - ay) * P(X, Y) + ax * (32 - ay) * P(X + 1, Y) + (32 - ax) * ay * P(X, Y + 1)
            + ax * ay * P(X + 1, Y + 1) + 512) >> 10


def mosaic(src, rec, S, luts=None, n_layers=2):
    """One image of adaisp_mosaic_u8 (launched with `n_layers`): uint8 [S,S,3]. `luts`: uint8 [n,768] or None."""
    v = layer(src, rec["layer"][0], S)
    if n_layers == 2 and int(rec["n_layers"]) == 2:
        mix = min(max(int(rec["mix"]), 0), 65536)
        v = (mix * v + (65536 - mix) * layer(src, rec["layer"][1], S)) >> 16
    v = v.astype(np.uint8)
    k = int(rec["lut"])
    return colour(v, luts[k]) if luts is not None and 0 <= k < len(luts) else v


def batch(src, recs, S, luts=None, n_layers=2):
    return np.stack([mosaic(src, r, S, luts, n_layers) for r in recs])
