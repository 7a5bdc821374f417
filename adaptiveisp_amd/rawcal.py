"""Calibration of a real sensor for the raw-capture path, host only: what adaisp_raw_correct (include/adaisp.h) is told.

Everything here is keyed by POSITION k = 2 * (y & 1) + (x & 1) in the sensor's 2 x 2 tile, the order of the letters in the
colour filter's name ("RGGB": k = 0 red, 1 and 2 green, 3 blue), which is how cameras report black levels and how DNG lays
out gain maps; `cfa` only says which sensor a calibration belongs to.

  RawCalibration         black levels, white level, a lens-shading gain grid, a defect threshold; one .npz
  from_frames            the same from dark frames and flat-field frames
  read_sidecar           per-capture metadata: <stem>.json beside <stem>.npy
  fill_rawfix            one adaisp_rawfix_desc record (the two divisions of the interface are the host's, in float64)
  python -m adaptiveisp_amd.rawcal --dark DIR --flat DIR --cfa RGGB --white 4095 --grid 13 17 --dpc 40 --out cal.npz
"""
import argparse
import json
import os

import numpy as np

CFA_NAMES = ("RGGB", "GRBG", "GBRG", "BGGR")
GAIN_FLOOR = 2.0 ** -6                            # a shading gain under this is a broken table, not a lens


def _four(value, field):
    """`value` (a number, or four numbers in 2 x 2 order) as float64 [4]; ValueError naming `field`."""
    try:
        a = np.asarray(value, np.float64)
    except (TypeError, ValueError):
        raise ValueError(f"{field}: a number or four numbers in 2 x 2 order, got {value!r}") from None
    if isinstance(value, (bool, str)) or a.dtype == object or a.shape not in ((), (4,)) or not np.isfinite(a).all():
        raise ValueError(f"{field}: a finite number or four finite numbers in 2 x 2 order, got {value!r}")
    return np.broadcast_to(a, (4,)).copy()


class RawCalibration:
    """black: None (the run's black level), a number or four numbers in 2 x 2 order; white: None (the run's white level)
    or a number above every black level; shading: None or an fp32 [4, gh, gw] array of finite gains >= GAIN_FLOOR, the
    grid's corners on the plane's corners whatever the plane's size; dpc: None (no defect correction) or an integer >= 0,
    the defect threshold in input counts; cfa: the sensor's colour filter."""

    def __init__(self, black, white, shading=None, dpc=None, cfa="RGGB"):
        self.black = None if black is None else _four(black, "black")
        if self.black is not None and (self.black < 0).any():
            raise ValueError(f"black: levels must be >= 0, got {black!r}")
        if white is None:
            self.white = None
        else:
            if isinstance(white, (bool, str)) or np.ndim(white) != 0 or not np.isfinite(float(white)):
                raise ValueError(f"white: one finite number, got {white!r}")
            self.white = float(white)
            if self.white <= 0 or (self.black is not None and self.white <= self.black.max()):
                raise ValueError(f"white: {white!r} must lie above every black level")
        if shading is None:
            self.shading = None
        else:
            s = np.asarray(shading)
            if s.dtype.kind not in "fiu" or s.ndim != 3 or s.shape[0] != 4 or min(s.shape[1:]) < 2:
                raise ValueError(f"shading: a [4, gh, gw] array of gains with gh, gw >= 2, got shape {s.shape}")
            s = np.ascontiguousarray(s, np.float32)
            if not np.isfinite(s).all() or (s < GAIN_FLOOR).any():
                raise ValueError(f"shading: gains must be finite and >= {GAIN_FLOOR}")
            self.shading = s
        if dpc is None:
            self.dpc = None
        else:
            if isinstance(dpc, bool) or not isinstance(dpc, (int, np.integer)) or dpc < 0 or dpc > 2 ** 31 - 1:
                raise ValueError(f"dpc: None or an integer >= 0, got {dpc!r}")
            self.dpc = int(dpc)
        if not isinstance(cfa, str) or cfa.upper() not in CFA_NAMES:
            raise ValueError(f"cfa: one of {list(CFA_NAMES)}, got {cfa!r}")
        self.cfa = cfa.upper()
        self.source = None                        # the file it was loaded from

    # ---------------------------------------------------------------------------------------------------- file
    def save(self, path):
        """One .npz holding only these arrays: cfa, and black / white / shading / dpc where they are set."""
        arrays = dict(cfa=np.array(self.cfa))
        if self.black is not None:
            arrays["black"] = self.black
        if self.white is not None:
            arrays["white"] = np.float64(self.white)
        if self.shading is not None:
            arrays["shading"] = self.shading
        if self.dpc is not None:
            arrays["dpc"] = np.int64(self.dpc)
        with open(path, "wb") as f:               # a file object: np.savez appends no ".npz" of its own
            np.savez(f, **arrays)

    @classmethod
    def load(cls, path):
        try:
            with np.load(path, allow_pickle=False) as z:
                got = {k: z[k] for k in z.files}
        except (OSError, ValueError, EOFError) as e:
            raise ValueError(f"{path}: not a calibration file ({e})") from None
        extra = sorted(set(got) - {"cfa", "black", "white", "shading", "dpc"})
        if extra or "cfa" not in got:
            raise ValueError(f"{path}: not a calibration file (arrays {sorted(got)})")
        try:
            cal = cls(got.get("black"), None if "white" not in got else float(got["white"]), got.get("shading"),
                      None if "dpc" not in got else int(got["dpc"]), str(got["cfa"]))
        except (TypeError, ValueError) as e:
            raise ValueError(f"{path}: {e}") from None
        cal.source = str(path)
        return cal

    def with_dpc(self, dpc):
        """The same calibration with another defect threshold."""
        cal = RawCalibration(self.black, self.white, self.shading, dpc, self.cfa)
        cal.source = self.source
        return cal

    def describe(self):
        parts = []
        if self.black is not None:
            parts.append("black " + " ".join(f"{b:g}" for b in self.black))
        if self.white is not None:
            parts.append(f"white {self.white:g}")
        if self.shading is not None:
            parts.append(f"shading {self.shading.shape[1]}x{self.shading.shape[2]}")
        if self.dpc is not None:
            parts.append(f"dpc {self.dpc}")
        name = os.path.basename(self.source) + ": " if self.source else ""
        return name + (", ".join(parts) if parts else "nothing set")

    # ---------------------------------------------------------------------------------------------------- estimate
    @classmethod
    def from_frames(cls, dark, flat, cfa="RGGB", grid=(13, 17), max_gain=8.0, white=None, dpc=None):
        """dark, flat: lists of uint16 planes of one size. black = the per-position mean of the dark frames. The flat
        frames are averaged, the black subtracted, and each position sampled at the grid's nodes (node (i, j) sits at
        y = i (H - 1) / (gh - 1), x = j (W - 1) / (gw - 1)): the value at a node is the mean of that position's samples in
        the window centred on the node, one grid cell wide, clipped to the plane (the nearest sample of the position when
        the window holds none). gain = the position's largest node value / the node's value, clamped to [1, max_gain].
        float64 throughout, one cast to fp32 at the end."""
        frames = {}
        for name, lst in (("dark", dark), ("flat", flat)):
            lst = [np.asarray(p) for p in lst]
            if not lst:
                raise ValueError(f"{name}: no frames")
            for p in lst:
                if p.ndim != 2 or p.dtype != np.uint16 or p.shape != lst[0].shape or min(p.shape) < 2:
                    raise ValueError(f"{name}: uint16 planes of one size, at least 2 x 2; got {p.dtype} {p.shape}")
            frames[name] = np.mean([p.astype(np.float64) for p in lst], axis=0)
        if frames["dark"].shape != frames["flat"].shape:
            raise ValueError(f"dark frames are {frames['dark'].shape}, flat frames {frames['flat'].shape}")
        gh, gw = (int(v) for v in grid)
        if gh < 2 or gw < 2:
            raise ValueError(f"grid: at least 2 x 2, got {grid!r}")
        if not max_gain >= 1.0:
            raise ValueError(f"max_gain: at least 1, got {max_gain!r}")
        H, W = frames["dark"].shape
        black = np.array([frames["dark"][k >> 1::2, k & 1::2].mean() for k in range(4)])
        shading = np.empty((4, gh, gw), np.float64)
        for k in range(4):
            ky, kx = k >> 1, k & 1
            sub = frames["flat"][ky::2, kx::2] - black[k]
            rows = _windows(ky + 2 * np.arange(sub.shape[0]), H, gh)
            cols = _windows(kx + 2 * np.arange(sub.shape[1]), W, gw)
            node = np.array([[sub[r][:, c].mean() for c in cols] for r in rows])
            with np.errstate(divide="ignore", invalid="ignore"):
                g = node.max() / node
            shading[k] = np.clip(np.where(np.isfinite(g) & (node > 0), g, max_gain), 1.0, max_gain)
        return cls(black, white, shading.astype(np.float32), dpc, cfa)


def _windows(coords, n, g):
    """Per grid node, the indices (into `coords`, the plane coordinates of one position's samples along an axis of n
    samples) inside the window centred on the node, one cell wide; the nearest one when the window holds none."""
    cell = (n - 1) / (g - 1)
    out = []
    for i in range(g):
        c = i * cell
        idx = np.nonzero(np.abs(coords - c) <= cell / 2)[0]
        out.append(idx if idx.size else np.array([int(np.abs(coords - c).argmin())]))
    return out


# ------------------------------------------------------------------------------------------------------------ sidecars
def sidecar_path(path):
    return os.path.splitext(path)[0] + ".json"


def read_sidecar(path):
    """The metadata of the capture `path` (<stem>.npy): <stem>.json beside it, or None when there is none. A dict with any
    of black (float64 [4]), white (float), gains (three floats, R G B: the as-shot white balance); other keys of the file
    are not ours and are ignored. A malformed file raises ValueError naming it."""
    side = sidecar_path(path)
    if not os.path.isfile(side):
        return None
    try:
        with open(side) as f:
            doc = json.load(f)
    except (OSError, ValueError) as e:
        raise ValueError(f"{side}: not JSON ({e})") from None
    if not isinstance(doc, dict):
        raise ValueError(f"{side}: a JSON object is expected, got {type(doc).__name__}")
    meta = {}
    try:
        if "black_level" in doc:
            meta["black"] = _four(doc["black_level"], "black_level")
            if (meta["black"] < 0).any():
                raise ValueError(f"black_level: levels must be >= 0, got {doc['black_level']!r}")
        if "white_level" in doc:
            w = doc["white_level"]
            if isinstance(w, bool) or not isinstance(w, (int, float)) or not np.isfinite(w) or w <= 0:
                raise ValueError(f"white_level: one finite number above 0, got {w!r}")
            meta["white"] = float(w)
        if "gains" in doc:
            g = doc["gains"]
            if (not isinstance(g, list) or len(g) != 3
                    or any(isinstance(v, bool) or not isinstance(v, (int, float)) or not np.isfinite(v) for v in g)):
                raise ValueError(f"gains: three finite numbers (R, G, B), got {g!r}")
            meta["gains"] = tuple(float(v) for v in g)
    except ValueError as e:
        raise ValueError(f"{side}: {e}") from None
    return meta


def resolve(cal, meta, run_black, run_white, where="calibration"):
    """What one capture is corrected with: (black float64 [4], white_in): the sidecar's, else the calibration's, else the
    run's. ValueError (naming `where`) when the white level does not lie above every black level."""
    meta = meta or {}
    black = meta.get("black")
    if black is None:
        black = cal.black if cal is not None and cal.black is not None else np.full(4, float(run_black))
    white = meta.get("white")
    if white is None:
        white = cal.white if cal is not None and cal.white is not None else float(run_white)
    if not white > black.max():
        raise ValueError(f"{where}: white level {white:g} does not lie above the black levels {black.tolist()}")
    return black, white


def calibration_from_options(path, dpc, cfa):
    """What --raw-cal FILE and --raw-dpc N mean together: the file's calibration, with N as its threshold when given; N
    alone: a calibration that only corrects defects (levels: the run's); neither: None."""
    if path is None:
        return None if dpc is None else RawCalibration(None, None, dpc=dpc, cfa=cfa)
    cal = RawCalibration.load(path)
    return cal if dpc is None else cal.with_dpc(dpc)


# ------------------------------------------------------------------------------------------------------------ descriptor
def fill_rawfix(rec, shape, src_offset, dst_offset, black, scale, black_out, dpc, grid):
    """One record of _lib.RAWFIX_DESC (adaisp_rawfix_desc). shape: (src_h, src_w), each >= 2; black, scale: four numbers
    by position; dpc: None or < 0 for no defect correction; grid: None, or (word offset of the [4, gh, gw] table in the
    gains buffer, gh, gw). The steps are (g - 1) / (side - 1) in float64, cast once."""
    H, W = int(shape[0]), int(shape[1])
    rec["src_offset"], rec["dst_offset"], rec["src_h"], rec["src_w"] = src_offset, dst_offset, H, W
    if grid is None:
        rec["grid"], rec["grid_h"], rec["grid_w"], rec["step_y"], rec["step_x"] = -1, 0, 0, 0.0, 0.0
    else:
        words, gh, gw = grid
        rec["grid"], rec["grid_h"], rec["grid_w"] = words, gh, gw
        rec["step_y"] = np.float32((gh - 1) / (H - 1)) if H > 1 else 0.0
        rec["step_x"] = np.float32((gw - 1) / (W - 1)) if W > 1 else 0.0
    rec["black"] = np.asarray(black, np.float64).astype(np.float32)
    rec["scale"] = np.asarray(scale, np.float64).astype(np.float32)
    rec["black_out"] = np.float32(black_out)
    rec["dpc"] = -1 if dpc is None or dpc < 0 else int(dpc)
    return rec


def level_scale(black, white_in, black_out, white_out):
    """scale[k] = (white_out - black_out) / (white_in - black[k]): float64, cast once (fill_rawfix does the cast)."""
    return (float(white_out) - float(black_out)) / (float(white_in) - np.asarray(black, np.float64))


# ------------------------------------------------------------------------------------------------------------ command line
def _planes_of(folder):
    files = sorted(f for f in os.listdir(folder) if f.lower().endswith(".npy"))
    if not files:
        raise ValueError(f"{folder}: no .npy planes")
    out = []
    for f in files:
        p = np.load(os.path.join(folder, f), allow_pickle=False)
        if p.ndim != 2 or p.dtype != np.uint16:
            raise ValueError(f"{os.path.join(folder, f)}: a 2-D uint16 plane is expected, got {p.dtype} {p.shape}")
        out.append(p)
    return out


def build_parser():
    ap = argparse.ArgumentParser(prog="python -m adaptiveisp_amd.rawcal",
                                 description="Estimate a sensor calibration from dark and flat-field frames")
    ap.add_argument("--dark", required=True, help="folder of dark frames (.npy, 2-D uint16)")
    ap.add_argument("--flat", required=True, help="folder of flat-field frames of the same size")
    ap.add_argument("--cfa", default="RGGB", choices=CFA_NAMES)
    ap.add_argument("--white", type=float, required=True, help="the sensor's white level")
    ap.add_argument("--grid", type=int, nargs=2, default=(13, 17), metavar=("GH", "GW"), help="shading grid nodes")
    ap.add_argument("--max-gain", type=float, default=8.0)
    ap.add_argument("--dpc", type=int, default=None, help="defect threshold in counts (default: no defect correction)")
    ap.add_argument("--out", required=True, help="the .npz to write")
    return ap


def main(argv=None):
    ap = build_parser()
    a = ap.parse_args(argv)
    try:
        cal = RawCalibration.from_frames(_planes_of(a.dark), _planes_of(a.flat), a.cfa, tuple(a.grid), a.max_gain,
                                         white=a.white, dpc=a.dpc)
    except ValueError as e:
        ap.error(str(e))
    cal.save(a.out)
    print(f"{a.out}: {cal.describe()}")
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
