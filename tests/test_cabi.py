"""The C-ABI library loads and exports every symbol include/adaisp.h declares (no compute: no GPU here)."""
import ctypes
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _declared(header):
    text = open(os.path.join(ROOT, "include", header)).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"\b(ada(?:isp|yolo)_\w+)\s*\(", text)))


def test_libadaisp_exports_header_symbols():
    from adaptiveisp_amd import _lib
    L = _lib.load()
    names = _declared("adaisp.h")
    assert set(_lib.EXPORTS) <= set(names)
    for n in names:
        assert hasattr(L, n), f"libadaisp.so does not export {n}"
    assert L.adaisp_abi_version() == _lib.ABI_VERSION
    assert L.adaisp_strerror(0) == b"ok" and b"alias" in L.adaisp_strerror(-3)
    expect = {-1: 0, 0: 1, 1: 1, 2: 9, 3: 1, 4: 1, 5: 8, 6: 1, 7: 1, 8: 1, 9: 3, 10: 2, 11: 1, 12: 24, 13: -1}
    for op, n in expect.items():
        assert L.adaisp_num_params(op) == n


def test_argument_checks_without_gpu():
    from adaptiveisp_amd import _lib
    L = _lib.load()
    # null pointers / bad sizes are rejected before anything touches a device
    assert L.adaisp_process(0, None, None, None, 1, 1, 8, 8, 0, None) == -1
    assert L.adaisp_forward(None, None, None, None, None, 1, 1, 8, 8, 0, None) == -1
    assert L.adaisp_pool64(None, None, 1, 8, 8, None) == -1
    buf = (ctypes.c_float * 16)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    assert L.adaisp_process(99, p, p, p, 1, 1, 2, 2, 0, None) == -2          # unknown op
    assert L.adaisp_process(2, p, p, p, 1, 1, 2, 2, 0, None) == -1           # CCM needs 9 params, stride 1
    assert L.adaisp_process(3, p, p, p, 1, 1, 2, 2, 0, None) == -3           # stencil in place
    # the host-known-op form of the RL step: same checks as adaisp_process, and never in place (it may be a stencil step)
    q = ctypes.cast((ctypes.c_float * 16)(), ctypes.c_void_p)
    assert L.adaisp_forward_uniform(0, None, None, None, None, 1, 1, 8, 8, 0, None) == -1
    assert L.adaisp_forward_uniform(99, p, q, None, p, 1, 1, 2, 2, 0, None) == -2
    assert L.adaisp_forward_uniform(2, p, q, None, p, 1, 1, 2, 2, 0, None) == -1
    assert L.adaisp_forward_uniform(0, p, p, None, p, 1, 1, 2, 2, 0, None) == -3
    assert L.adaisp_forward_uniform(0, p, q, None, p, 1, 1, 2, 2, 0, None) == -4          # H, W < 3


def test_fused_pooling_geometry_is_host_side_and_total():
    """The cut of the fused-pooling kernels (isp_internal.h: PoolGeom), restated: every pixel column is owned by exactly one
    strip, every strip's read span covers what it owns and fits 64 lanes x 4 px, for the BASELINE sizes and awkward widths."""
    def win_lo(o, n): return (o * n) // 64
    def win_hi(o, n): return ((o + 1) * n + 63) // 64
    for W in (64, 68, 72, 100, 128, 200, 512, 640, 1000, 1280, 1920, 3840, 4096):
        geom = None
        for strips in range(1, 17):
            cps = (64 + strips - 1) // strips
            if (64 + cps - 1) // cps != strips:
                continue
            c0 = lambda s: min(s * cps, 64)                                            # noqa: E731
            lo = lambda s: W if c0(s) >= 64 else win_lo(c0(s), W) & ~3                  # noqa: E731
            end = lambda s: (win_hi(c0(s + 1) - 1, W) + 3) & ~3                         # noqa: E731
            if all(end(s) - lo(s) <= 256 for s in range(strips)):
                geom = (cps, strips, lo, end)
                break
        assert geom is not None, W
        cps, strips, lo, end = geom
        owned = []
        for s in range(strips):
            assert lo(s) % 4 == 0 and end(s) % 4 == 0 and lo(s) < end(s) <= W and end(s) >= lo(s + 1)
            for ox in range(min(s * cps, 64), min((s + 1) * cps, 64)):                 # its pool columns lie inside its span
                assert lo(s) <= win_lo(ox, W) and win_hi(ox, W) <= end(s)
            owned += list(range(lo(s), lo(s + 1)))
        assert owned == list(range(W)), W


def test_libadayolo_exports_header_symbols():
    from adaptiveisp_amd.yolo import _lib
    L = _lib.load()
    names = _declared("adayolo.h")
    assert set(_lib.EXPORTS) <= set(names)
    for n in names:
        assert hasattr(L, n), f"libadayolo.so does not export {n}"
    assert L.adayolo_abi_version() == _lib.ABI_VERSION
    assert not hasattr(L, "adayolo_debug_stamps")            # measurement builds are not in the shipped library


def test_adayolo_argument_checks_without_gpu():
    """Rejected before anything touches a device: null pointers, bad channel counts, kernel numbers that are not in the
    library (only the variants the tuning table may name exist: include/adayolo.h)."""
    from adaptiveisp_amd.yolo import _lib
    L = _lib.load()
    buf = (ctypes.c_float * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    conv = L.adayolo_conv_fwd_variant
    assert conv(None, 8, p, p, None, 0, p, 8, 1, 4, 4, 8, 8, 3, 1, 1, 0, None) == -1
    assert conv(p, 8, p, p, None, 0, p, 8, 1, 4, 4, 7, 8, 3, 1, 1, 0, None) == -2            # Cin % 8
    assert conv(p, 8, p, p, None, 0, p, 8, 1, 4, 4, 8, 8, 5, 1, 1, 0, None) == -2            # ksize 5
    for bogus in (1, 3, 13, 33, 41, 57, 66, 99):
        assert conv(p, 8, p, p, None, 0, p, 8, 1, 4, 4, 8, 8, 3, 1, 1, bogus, None) == -1, bogus
    assert L.adayolo_letterbox_pack(None, p, 8, 1, 4, 4, 4, 0, 0.5, None) == -1
    assert L.adayolo_letterbox_pack(p, p, 6, 1, 4, 4, 4, 0, 0.5, None) == -2


def test_detloss_argument_checks_without_gpu():
    """adayolo_detloss_fwd / _bwd (include/adayolo.h) refuse malformed argument blocks before any launch, and the
    ctypes mirror of the structs has the header's layout (88 / 424 bytes on LP64)."""
    from adaptiveisp_amd.yolo import _lib
    L = _lib.load()
    assert ctypes.sizeof(_lib.LossLayer) == 88 and ctypes.sizeof(_lib.LossArgs) == 424
    assert L.adayolo_detloss_fwd(None, None) == -1
    buf = (ctypes.c_float * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p).value
    a = _lib.LossArgs()
    a.nl, a.B, a.na, a.nc, a.no, a.loss, a.ticket = 1, 1, 3, 80, 85, p, p
    lay = a.layer[0]
    lay.raw, lay.cs, lay.ny, lay.nx, lay.tobj, lay.cnt, lay.part, lay.n = p, 256, 2, 2, p, p, p, 0
    lay.cs = 248                                               # narrower than na * no
    assert L.adayolo_detloss_fwd(ctypes.byref(a), None) == -2
    lay.cs = 256
    a.no = 84                                                  # no != nc + 5
    assert L.adayolo_detloss_fwd(ctypes.byref(a), None) == -1
    a.no = 85
    lay.n = 3                                                  # matches announced, no arrays
    assert L.adayolo_detloss_fwd(ctypes.byref(a), None) == -1
    lay.n = 0
    a.nc, a.no = 200, 205                                      # more than two classes per lane
    assert L.adayolo_detloss_fwd(ctypes.byref(a), None) == -2
    a.nc, a.no = 80, 85
    assert L.adayolo_detloss_bwd(ctypes.byref(a), None) == -1  # no upstream gradient
    a.grad_loss = p
    assert L.adayolo_detloss_bwd(ctypes.byref(a), None) == -2  # no gradient map
    lay.grad, lay.grad_cs = p, 252                             # not a multiple of 8
    assert L.adayolo_detloss_bwd(ctypes.byref(a), None) == -2


def test_chain_tables_without_gpu():
    """adayolo_conv_chain_tables (the workspace image adayolo_conv_chain_prepare uploads) for a 4-layer chain with fake device
    addresses: layer-major item order, one arrival counter per (layer, m-tile), and for EVERY tile the dependency window checked
    against a brute-force model — the set of producer m-tiles that hold a pixel one of the tile's taps reads (3x3 halo across
    image rows and image boundaries, stride 2 at the end) must be inside [in_lo, in_lo + in_n), and the residual rows' tile too."""
    import ctypes
    import numpy as np
    from adaptiveisp_amd.yolo import _lib
    L = _lib.load()
    B, H, W = 3, 21, 13                                       # M = 819: 4 m-tiles, images straddle tiles
    base = 0x10000000
    MB = 1 << 24
    x, w, b = base, base + 1 * MB, base + 2 * MB
    x0, h0, x1, h1, x2, y = (base + k * MB for k in range(3, 9))
    w2 = base + 10 * MB

    def layer(inp, cin, res, out, cout, s, out2=None, Hi=H, Wi=W):
        c = _lib.ChainLayer()
        c.in_, c.in_cstride, c.weight, c.bias, c.residual, c.res_cstride = inp, cin, w, b, res, 256 if res else 0
        c.out, c.out_cstride, c.B, c.H, c.W, c.Cin, c.Cout, c.ksize, c.stride, c.act = out, cout, B, Hi, Wi, cin, cout, 3, s, 1
        if out2:
            c.weight2, c.bias2, c.out2, c.out2_cstride, c.Cout2 = w2, b, out2, 128, 128
        return c
    specs = [layer(x, 64, None, x0, 256, 1, h0), layer(h0, 128, x0, x1, 256, 1, h1), layer(h1, 128, x1, x2, 256, 1),
             layer(x2, 256, None, y, 512, 2)]
    arr = (_lib.ChainLayer * 4)(*specs)
    nbytes = L.adayolo_conv_chain_workspace_bytes(arr, 4)
    assert nbytes > 0
    img = np.zeros(nbytes, np.uint8)
    info = (ctypes.c_int32 * 6)()
    assert L.adayolo_conv_chain_tables(arr, 4, img.ctypes.data_as(ctypes.c_void_p), nbytes, info) == 0
    total, ndone, off_layers, off_items, off_deps, _ = list(info)
    M = B * H * W
    mt = (M + 255) // 256
    Ho, Wo = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    M3 = B * Ho * Wo
    mt3 = (M3 + 255) // 256
    assert total == 3 * mt + mt3 * 2 and ndone == 3 * mt + mt3
    items = img[off_items:off_items + 16 * total].view(np.int32).reshape(total, 4)
    deps = img[off_deps:off_deps + 16 * total].view(np.int32).reshape(total, 4)
    assert (img[:64 + 4 * ndone] == 0).all()
    # layer-major order, tiles ascending; counters: one per (layer, m-tile)
    want_items = [(l, t, l * mt + t) for l in range(3) for t in range(mt)] + [(3, t, 3 * mt + t // 2) for t in range(mt3 * 2)]
    assert [tuple(r[:3]) for r in items.tolist()] == want_items
    src_in, src_res = [None, 0, 1, 2], [None, 0, 1, None]
    for (l, lid, flag, _), (in_lo, inn, res_lo, rnn) in zip(items.tolist(), deps.tolist()):
        s, (Hq, Wq, Mq) = (2, (Ho, Wo, M3)) if l == 3 else (1, (H, W, M))
        m_tile = lid // (2 if l == 3 else 1)
        need = set()
        for m in range(m_tile * 256, min(m_tile * 256 + 256, Mq)):
            bb, rem = divmod(m, Hq * Wq)
            ho, wo = divmod(rem, Wq)
            for kh in range(3):
                for kw in range(3):
                    hi, wi = ho * s - 1 + kh, wo * s - 1 + kw
                    if 0 <= hi < H and 0 <= wi < W:
                        need.add(((bb * H + hi) * W + wi) // 256)
        if src_in[l] is None:
            assert inn == 0
        else:
            n_in, need_in = inn >> 16, inn & 0xFFFF
            lo = in_lo - src_in[l] * mt
            assert need_in == 1 and 1 <= n_in <= 32 and 0 <= lo and lo + n_in <= mt
            assert need <= set(range(lo, lo + n_in)), (l, lid, sorted(need), lo, n_in)
            assert n_in <= len(need) + 2                     # a window, not "everything"
        if src_res[l] is None:
            assert rnn == 0
        else:
            assert res_lo == src_res[l] * mt + m_tile and rnn == (1 << 16) | 1
    # an item only ever waits for counters of EARLIER layers (deadlock freedom of the hand-out order)
    for (l, _, flag, _), (in_lo, inn, res_lo, rnn) in zip(items.tolist(), deps.tolist()):
        if inn:
            assert in_lo + (inn >> 16) <= l * mt
        if rnn:
            assert res_lo < l * mt
    # argument checks
    assert L.adayolo_conv_chain_fwd(arr, 4, None, 0, None) == -1
    assert L.adayolo_conv_chain_prepare(arr, 4, None, 0) == -1
    bad = (_lib.ChainLayer * 4)(*specs)
    bad[2].out = x0                                           # writes what layer 1 reads
    assert L.adayolo_conv_chain_workspace_bytes(bad, 4) == 0


def test_chain_tables_mixed_tiles_without_gpu():
    """A chain that mixes the two tile kinds, as the detector's C = 512 stage does: 3x3 128 -> 512 on 256 x 256 tiles (two n-tiles
    per m-tile), Bottleneck.cv1 1x1 512 -> 256 on 256 x 128 tiles (two n-tiles), Bottleneck.cv2 3x3 256 -> 512 + shortcut on
    256 x 256 tiles. Counters are per (layer, m-tile) and count n-tiles: a consumer needs ALL n-tiles of every producer m-tile
    in its window (need = the producer's n-tile count); a 1x1 layer's window is its own pixels."""
    import ctypes
    import numpy as np
    from adaptiveisp_amd.yolo import _lib
    L = _lib.load()
    B, H, W = 2, 19, 27                                       # M = 1026: 5 m-tiles, the last one 2 pixels
    base, MB = 0x20000000, 1 << 24
    x, w, b, y0, h, y1 = (base + k * MB for k in range(6))

    def layer(inp, cin, res, out, cout, k, tile):
        c = _lib.ChainLayer()
        c.in_, c.in_cstride, c.weight, c.bias, c.residual, c.res_cstride = inp, cin, w, b, res, cout if res else 0
        c.out, c.out_cstride, c.B, c.H, c.W, c.Cin, c.Cout, c.ksize, c.stride, c.act, c.tile = out, cout, B, H, W, cin, cout, k, 1, 1, tile
        return c
    specs = [layer(x, 128, None, y0, 512, 3, 0), layer(y0, 512, None, h, 256, 1, 1), layer(h, 256, y0, y1, 512, 3, 0)]
    arr = (_lib.ChainLayer * 3)(*specs)
    nbytes = L.adayolo_conv_chain_workspace_bytes(arr, 3)
    assert nbytes > 0
    img = np.zeros(nbytes, np.uint8)
    info = (ctypes.c_int32 * 6)()
    assert L.adayolo_conv_chain_tables(arr, 3, img.ctypes.data_as(ctypes.c_void_p), nbytes, info) == 0
    total, ndone, off_layers, off_items, off_deps, _ = list(info)
    mt = (B * H * W + 255) // 256
    assert (total, ndone) == (mt * 2 * 3, mt * 3)
    items = img[off_items:off_items + 16 * total].view(np.int32).reshape(total, 4).tolist()
    deps = img[off_deps:off_deps + 16 * total].view(np.int32).reshape(total, 4).tolist()
    assert [tuple(r[:3]) for r in items] == [(l, t, l * mt + t // 2) for l in range(3) for t in range(2 * mt)]
    for (l, lid, flag, _), (in_lo, inn, res_lo, rnn) in zip(items, deps):
        m_tile = lid // 2
        if l == 0:
            assert inn == 0 and rnn == 0
            continue
        n_in, need_in = inn >> 16, inn & 0xFFFF
        assert need_in == 2                                   # both n-tiles of every producer m-tile
        lo = in_lo - (l - 1) * mt
        if l == 1:                                            # 1x1: exactly its own m-tile
            assert (lo, n_in) == (m_tile, 1) and rnn == 0
        else:
            need = set()
            for m in range(m_tile * 256, min(m_tile * 256 + 256, B * H * W)):
                bb, rem = divmod(m, H * W)
                ho, wo = divmod(rem, W)
                need |= {((bb * H + hi) * W + wi) // 256 for hi in range(ho - 1, ho + 2) for wi in range(wo - 1, wo + 2)
                         if 0 <= hi < H and 0 <= wi < W}
            assert need <= set(range(lo, lo + n_in)) and n_in <= len(need) + 2
            assert (res_lo, rnn) == (m_tile, (1 << 16) | 2)    # the shortcut: layer 0's m-tile, both its n-tiles
    # a fused layer must be on the 256 x 256 tile; the 256 x 128 tile takes Cout % 128
    bad = (_lib.ChainLayer * 3)(*specs)
    bad[1].tile = 0                                           # Cout 256 on 256 x 256 tiles is fine ...
    assert L.adayolo_conv_chain_workspace_bytes(bad, 3) > 0
    bad[1].tile = 2
    assert L.adayolo_conv_chain_workspace_bytes(bad, 3) == 0
    bad[1].tile, bad[1].Cout, bad[1].out_cstride = 1, 192, 192
    assert L.adayolo_conv_chain_workspace_bytes(bad, 3) == 0


# ---- every argument rule of libadayolo.so's entry points, as a table --------------------------------------------------------
# One well-formed call per entry (parameters in the header's order; never made: it would launch) and that entry's single
# faults. A case = one fault, or two faults on different parameters; every case is refused by the entry's own checks, before
# any launch, so the fake addresses are never read. _REJECT_CODES holds, per entry and in the order _reject_cases yields,
# the code each case returned from the library as built from the commit BEFORE the argument handling of yolo_api.hip was
# factored ('1' = ADAYOLO_EINVAL, '2' = ADAYOLO_ESHAPE, '0' = a size of 0 from the *_bytes entries):
#     ADAYOLO_LIB=<that commit's libadayolo.so> python tests/test_cabi.py
# prints the table. Which of two faults is reported is part of the contract.
_A, _B_, _C = 0x10000000, 0x20000000, 0x30000000              # fake device addresses (in / out / the other tensors)
_SK = 100 + 4                                                  # ADAYOLO_SPLITK_BASE + S
_DROP = object()                                               # a parameter this entry does not have


def _conv(extra_ptrs=(), tail=(), **over):
    g = dict(in_=_A, in_cs=128, weight=_C, bias=_C, residual=_C, res_cs=128, out=_B_, out_cs=128)
    g.update(extra_ptrs)
    g.update(B=2, H=16, W=16, Cin=128, Cout=128, ksize=3, stride=1, act=1)
    g.update(tail)
    g.update(over)
    return {k: v for k, v in g.items() if v is not _DROP}


_CONV_FAULTS = [dict(in_=None), dict(weight=None), dict(bias=None), dict(out=None), dict(B=0), dict(H=-1), dict(W=0), dict(Cin=0),
                dict(Cout=-8), dict(ksize=2), dict(ksize=5), dict(stride=3), dict(stride=0), dict(Cin=124), dict(Cout=100),
                dict(in_cs=132), dict(in_cs=120), dict(out_cs=130), dict(out_cs=64), dict(res_cs=12), dict(res_cs=120),
                dict(act=2), dict(act=-1), dict(B=4, H=32768, W=32768)]
_PRE_FAULTS = [dict(pre=None), dict(pre_cs=132), dict(pre_cs=64)]
_STEM = dict(img=_A, weight=_C, bias=_C, out=_B_, out_cs=32, B=2, H=30, W=64, Hp=32, pad_top=1, pad_value=0.5, Cout=32)
_STEM_FAULTS = [dict(img=None), dict(weight=None), dict(bias=None), dict(out=None), dict(B=0), dict(H=0), dict(W=-1), dict(Hp=29),
                dict(pad_top=-1), dict(pad_top=3), dict(Cout=64), dict(out_cs=36), dict(out_cs=24), dict(B=65536)]
_BNECK = dict(x=_A, x_cs=256, w1=_C, b1=_C, w2=_C, b2=_C, out=_B_, out_cs=256, B=1, H=16, W=16)
_BNECK_FAULTS = [dict(x=None), dict(w1=None), dict(b1=None), dict(w2=None), dict(b2=None), dict(out=None), dict(out=_A), dict(B=0),
                 dict(H=0), dict(W=-2), dict(x_cs=260), dict(out_cs=252), dict(x_cs=128), dict(out_cs=64)]
_VARIANTS_NOT_IN_LIB = [dict(variant=v) for v in (1, 3, 13, 33, 41, 57, 66, 99, -1)]
_SPLIT_OUTSIDE = [dict(variant=100), dict(variant=101), dict(variant=117), dict(variant=200)]

_ENTRIES = {
    "adayolo_conv_fwd_variant": (_conv(tail=dict(variant=60, stream=None)), _CONV_FAULTS + _VARIANTS_NOT_IN_LIB + _SPLIT_OUTSIDE + [dict(variant=_SK)]),
    "adayolo_conv_fwd": (_conv(tail=dict(stream=None)), _CONV_FAULTS),
    "adayolo_conv_fused1x1_fwd": (
        _conv(Cout=256, out_cs=256, res_cs=256, tail=dict(weight2=_C, bias2=_C, out2=_C + 0x1000000, out2_cs=128, Cout2=128, stream=None)),
        _CONV_FAULTS + [dict(weight2=None), dict(bias2=None), dict(out2=None), dict(Cout=128), dict(Cout2=256), dict(Cin=96),
                        dict(out2_cs=132), dict(out2_cs=64), dict(out_cs=128), dict(res_cs=128)]),
    "adayolo_conv1x1_stream_fwd": (
        dict(in_=_A, in_cs=256, weight=_C, bias=_C, out=_B_, out_cs=256, B=2, H=16, W=16, Cin=256, Cout=256, act=1, stream=None),
        [f for f in _CONV_FAULTS if not set(f) & {"ksize", "stride", "residual", "res_cs"}] + [dict(out=_A)]),
    "adayolo_bottleneck256_fwd": (dict(_BNECK, stream=None), _BNECK_FAULTS + [dict(B=4, H=32768, W=32768)]),
    "adayolo_bottleneck_ws_fwd": (dict(_BNECK, x_cs=128, out_cs=128, C=128, stream=None),
                                  [f for f in _BNECK_FAULTS if f not in (dict(x_cs=128), dict(out_cs=252))] + [dict(C=256), dict(C=0), dict(out_cs=120)]),
    "adayolo_conv_keep_fwd": (_conv(dict(pre=_C, pre_cs=128), tail=dict(variant=60, stream=None)),
                              _CONV_FAULTS + _PRE_FAULTS + _VARIANTS_NOT_IN_LIB + _SPLIT_OUTSIDE +
                              [dict(variant=v) for v in (0, 2, 40, 50, 90, _SK)]),
    "adayolo_conv_splitk_workspace_bytes": (
        dict(B=8, H=16, W=16, Cin=1024, Cout=512, ksize=3, stride=1, variant=_SK),
        [dict(B=0), dict(H=-1), dict(W=0), dict(Cin=0), dict(Cout=-8), dict(ksize=0), dict(ksize=4), dict(stride=3), dict(stride=0)] +
        _SPLIT_OUTSIDE + [dict(variant=v) for v in (0, 2, 60)] + [dict(Cin=96), dict(Cout=192), dict(variant=107), dict(B=4, H=32768, W=32768)]),
    "adayolo_conv_splitk_fwd": (
        _conv(dict(pre=_C, pre_cs=512), B=8, Cin=1024, Cout=512, in_cs=1024, out_cs=512, res_cs=512,
              tail=dict(variant=_SK, workspace=_C, workspace_bytes=1 << 30, stream=None)),
        [dict(f, **{k: {124: 1020, 100: 500, 132: 1028, 120: 1016, 130: 514, 64: 256}.get(v, v) if k in ("Cin", "Cout", "in_cs", "out_cs") else v
                    for k, v in f.items()}) for f in _CONV_FAULTS if "res_cs" not in f] +
        [dict(res_cs=12), dict(res_cs=504), dict(pre_cs=516), dict(pre_cs=256), dict(workspace=None), dict(workspace_bytes=4096),
         dict(Cin=96, in_cs=1024), dict(variant=107)] + _SPLIT_OUTSIDE + [dict(variant=v) for v in (0, 2, 60)]),
    "adayolo_conv_dsilu_fwd": (
        _conv(dict(pre=_C, pre_cs=128, grad_pre=_C + 0x2000000, gp_cs=128), act=_DROP,
              tail=dict(variant=60, workspace=None, workspace_bytes=0, stream=None)),
        [f for f in _CONV_FAULTS if "act" not in f and f != dict(out=None)] + _PRE_FAULTS +
        [dict(grad_pre=None), dict(gp_cs=132), dict(gp_cs=64), dict(out=None, gp_cs=64), dict(variant=_SK), dict(variant=107)] +
        _VARIANTS_NOT_IN_LIB + _SPLIT_OUTSIDE + [dict(variant=v) for v in (0, 2, 40, 50, 90)]),
    "adayolo_conv_s2grad_fwd": (
        dict(grad_out=_A, go_cs=128, weight4=_C, bias4=_C, residual=_C, res_cs=64, grad_in=_B_, gi_cs=64, pre=_C, pre_cs=64,
             grad_pre=_C + 0x2000000, gp_cs=64, B=2, Ho=8, Wo=8, Cout=128, Cin=64, variant=60, workspace=None, workspace_bytes=0, stream=None),
        [dict(grad_out=None), dict(weight4=None), dict(bias4=None), dict(grad_in=None, grad_pre=None), dict(pre=None), dict(B=0),
         dict(Ho=-1), dict(Wo=0), dict(Cin=0), dict(Cout=-8), dict(Cin=60), dict(Cout=100), dict(go_cs=132), dict(go_cs=64),
         dict(gi_cs=68), dict(gi_cs=32), dict(res_cs=12), dict(res_cs=56), dict(pre_cs=68), dict(pre_cs=32), dict(gp_cs=68),
         dict(gp_cs=32), dict(B=4, Ho=32768, Wo=32768), dict(variant=_SK), dict(variant=107)] +
        _VARIANTS_NOT_IN_LIB + _SPLIT_OUTSIDE + [dict(variant=v) for v in (0, 2, 40, 50, 80, 85, 90)]),
    "adayolo_stem_fwd": (dict(_STEM, stream=None), _STEM_FAULTS),
    "adayolo_stem_fwd_act": (dict(_STEM, act=0, stream=None), _STEM_FAULTS + [dict(act=2), dict(act=-1)]),
    "adayolo_stem_keep_fwd": (
        dict(img=_A, weight=_C, bias=_C, out=_B_, out_cs=32, pre=_C, pre_cs=32, B=2, H=30, W=64, Hp=32, pad_top=1, pad_value=0.5, Cout=32, stream=None),
        _STEM_FAULTS + [dict(pre=None), dict(pre_cs=36), dict(pre_cs=24)]),
    "adayolo_letterbox_pack": (dict(img=_A, out=_B_, out_cs=8, B=2, H=30, W=64, Hp=32, pad_top=1, pad_value=0.5, stream=None),
                               [dict(img=None), dict(out=None), dict(B=0), dict(H=0), dict(W=-1), dict(Hp=29), dict(pad_top=-1), dict(pad_top=3),
                                dict(out_cs=6), dict(out_cs=0), dict(B=65536), dict(H=65536, Hp=65536)]),
    "adayolo_stem_down_fwd": (
        dict(img=_A, w_stem=_C, b_stem=_C, w_down=_C, b_down=_C, out=_B_, out_cs=64, B=2, H=30, W=64, Hp=32, pad_top=1, pad_value=0.5,
             w_next=_C, b_next=_C, out_next=_C + 0x2000000, out_next_cs=32, stream=None),
        [dict(img=None), dict(w_stem=None), dict(b_stem=None), dict(w_down=None), dict(b_down=None), dict(out=None), dict(b_next=None),
         dict(out_next=None), dict(out_next_cs=36), dict(out_next_cs=24), dict(B=0), dict(H=0), dict(W=-1), dict(Hp=29), dict(pad_top=-1),
         dict(pad_top=3), dict(H=31, Hp=33), dict(W=63), dict(out_cs=68), dict(out_cs=32), dict(B=65536)]),
    "adayolo_silu_fwd": (dict(pre=_A, pre_cs=64, residual=_C, res_cs=64, out=_B_, out_cs=64, npix=100, C=64, stream=None),
                         [dict(pre=None), dict(out=None), dict(npix=0), dict(npix=-5), dict(C=0), dict(C=60), dict(pre_cs=68), dict(pre_cs=32),
                          dict(out_cs=68), dict(out_cs=32), dict(res_cs=68), dict(res_cs=32)]),
    "adayolo_silu_bwd": (
        dict(grad_out=_A, go_cs=64, pre=_C, pre_cs=64, grad_pre=_B_, gp_cs=64, grad_res=_C + 0x2000000, gr_cs=64, accumulate_res=0, npix=100, C=64, stream=None),
        [dict(grad_out=None), dict(npix=0), dict(grad_pre=None, grad_res=None), dict(pre=None), dict(C=0), dict(C=60), dict(go_cs=68),
         dict(go_cs=32), dict(pre_cs=68), dict(pre_cs=32), dict(gp_cs=68), dict(gp_cs=32), dict(gr_cs=68), dict(gr_cs=32)]),
    "adayolo_zero_insert2x": (dict(in_=_A, in_cs=64, out=_B_, out_cs=64, B=2, Ho=8, Wo=8, H=16, W=15, C=64, stream=None),
                              [dict(in_=None), dict(out=None), dict(B=0), dict(Ho=0), dict(Wo=-1), dict(H=0), dict(W=-1), dict(C=0), dict(C=60),
                               dict(in_cs=68), dict(in_cs=32), dict(out_cs=68), dict(out_cs=32), dict(Ho=9), dict(Wo=7)]),
    "adayolo_upsample2x_bwd": (dict(grad_out=_A, go_cs=64, grad_in=_B_, gi_cs=64, accumulate=0, B=2, H=8, W=8, C=64, stream=None),
                               [dict(grad_out=None), dict(grad_in=None), dict(B=0), dict(H=0), dict(W=-1), dict(C=0), dict(C=60), dict(go_cs=68),
                                dict(go_cs=32), dict(gi_cs=68), dict(gi_cs=32)]),
    "adayolo_image_grad": (dict(grad_nhwc=_A, g_cs=8, grad_img=_B_, B=2, H=30, W=64, Hp=32, pad_top=1, stream=None),
                           [dict(grad_nhwc=None), dict(grad_img=None), dict(B=0), dict(H=0), dict(W=-1), dict(Hp=29), dict(pad_top=-1),
                            dict(pad_top=3), dict(g_cs=2), dict(g_cs=5)]),
    "adayolo_upsample2x": (dict(in_=_A, in_cs=64, out=_B_, out_cs=64, B=2, H=8, W=8, C=64, stream=None),
                           [dict(in_=None), dict(out=None), dict(B=0), dict(H=0), dict(W=-1), dict(C=0), dict(C=60), dict(in_cs=68),
                            dict(in_cs=32), dict(out_cs=68), dict(out_cs=32)]),
    "adayolo_detect_decode": (
        dict(raw=_A, raw_cs=256, pred=_B_, pred_rows=1000, row_offset=100, anchors_px=_C, det_stride=8.0, B=2, ny=8, nx=8, na=3, no=85, stream=None),
        [dict(raw=None), dict(pred=None), dict(anchors_px=None), dict(B=0), dict(ny=0), dict(nx=-1), dict(na=0), dict(no=4), dict(raw_cs=248),
         dict(row_offset=-1), dict(row_offset=900), dict(pred_rows=200)]),
    "adayolo_nms": (dict(boxes=_A, n=100, iou_thres=0.5, max_det=300, workspace=_C, keep=_B_, num_keep=_B_ + 4096, stream=None),
                    [dict(n=-1), dict(max_det=0), dict(keep=None), dict(num_keep=None), dict(boxes=None), dict(workspace=None), dict(n=120001),
                     dict(iou_thres=-0.1), dict(iou_thres=1.5), dict(iou_thres=float("nan"))]),
}


def _chain_cases():
    """A well-formed two-layer chain (3x3 64 -> 256 with the next block's 1x1 fused, then 3x3 128 -> 256 + shortcut on 256 x 128
    tiles) with one or two fields of its SECOND layer broken."""
    from adaptiveisp_amd.yolo import _lib
    x, h, y0, y1 = _A, _B_, _B_ + 0x4000000, _B_ + 0x8000000
    faults = [dict(in_=None), dict(weight=None), dict(bias=None), dict(out=None), dict(B=0), dict(H=-1), dict(Cin=0), dict(ksize=5),
              dict(stride=3), dict(Cin=120), dict(Cin=96, in_cstride=96), dict(Cout=192), dict(in_cstride=132), dict(out_cstride=64),
              dict(res_cstride=12), dict(act=2), dict(tile=2), dict(tile=0, Cout=128, out_cstride=128), dict(out=x), dict(out=h),
              dict(residual=y1), dict(weight2=_C, tile=1), dict(weight2=_C, tile=0), dict(weight2=_C, tile=0, bias2=_C, out2=y1 + 0x4000000, Cout2=64)]
    cases = faults + [dict(f, **g) for i, f in enumerate(faults) for g in faults[i + 1:] if not set(f) & set(g)]
    for c in cases:
        l0, l1 = _lib.ChainLayer(), _lib.ChainLayer()
        for k, v in dict(in_=x, in_cstride=64, weight=_C, bias=_C, out=y0, out_cstride=256, B=2, H=16, W=16, Cin=64, Cout=256, ksize=3,
                         stride=1, act=1, weight2=_C, bias2=_C, out2=h, out2_cstride=128, Cout2=128, tile=0).items():
            setattr(l0, k, v)
        for k, v in dict(dict(in_=h, in_cstride=128, weight=_C, bias=_C, residual=y0, res_cstride=256, out=y1, out_cstride=256, B=2, H=16,
                              W=16, Cin=128, Cout=256, ksize=3, stride=1, act=1, tile=1), **c).items():
            setattr(l1, k, v)
        yield (_lib.ChainLayer * 2)(l0, l1)


def _reject_codes(L, name):
    """The codes of every case of one entry, as a string of _REJECT_CODES' letters ('?': not a rejection)."""
    letter = {-1: "1", -2: "2", 0: "0"}
    if name == "chain":
        img = (ctypes.c_char * 64)()
        out = []
        for arr in _chain_cases():
            out += [letter.get(L.adayolo_conv_chain_workspace_bytes(arr, 2), "?"),
                    letter.get(L.adayolo_conv_chain_tables(arr, 2, img, 64, None), "?").replace("0", "?"),
                    letter.get(L.adayolo_conv_chain_prepare(arr, 2, _C, 1 << 30), "?").replace("0", "?"),
                    letter.get(L.adayolo_conv_chain_fwd(arr, 2, _C, 1 << 30, None), "?").replace("0", "?")]   # never prepared
        return "".join(out)
    good, faults = _ENTRIES[name]
    cases = faults + [dict(f, **g) for i, f in enumerate(faults) for g in faults[i + 1:] if not set(f) & set(g)]
    sized = name.endswith("_bytes")
    out = []
    for c in cases:
        assert set(c) <= set(good), (name, c)
        rc = getattr(L, name)(*dict(good, **c).values())
        out.append(letter.get(rc, "?") if sized == (rc == 0) else "?")
    return "".join(out)


_REJECT_CODES = {
    "adayolo_conv_fwd_variant": (
        "111111111222222222222112111111111111111111111111111111111111111111111111111111111111111111111111111111111111111111111111"
        "111111111111111111111111111111111111111111111111111111111111111111111111111111111111111111111111111111111111111111111111"
        "111111111111111111111111111111111111111111111111111111111111111111111111111111111111111111222222222222222222222222222222"
        "222222222222222222222222222222222222222222222222222222222222222222222222222222222222222222222222222222222222222222222222"
        "222222222222222222222222222222222222222222222222222222222222222222222222222222222222222222222222222222222222222222211111"
        "111111111111111111111111122222222222222"
    ),
    "adayolo_conv_fwd": (
        "111111111222222222222112111111111111111111111111111111111111111111111111111111111111111111111111111111111111111111111111"
        "111111111111111111111111111111111111111111111111111111111111111111111122222222222222222222222222222222222222222222222222"
        "2222222222222222222222222222222222222222222222211"
    ),
    "adayolo_conv_fused1x1_fwd": (
        "111111111222222222222112111222222211111111111111111111111111111111111111111111111111111111111111111111111111111111111111"
        "111111111111111111111111111111111111111111111111111111111111111111111111111111111111111111111111111111111111111111111111"
        "111111111111111111111111111111111111111111111111222222222222211122222222222222222222111222222222222222222111222222222222"
        "222222111222222222222222221112222222222222221112222222222222111222222222222221112222222222221112222222222211122222222211"
        "12222222221112222221111222222211112222222111222222211111111111111111111111122222222222222222222"
    ),
    "adayolo_conv1x1_stream_fwd": (
        "111111111222222112111111111111111111111111111111111111111111111111111111111111111111111111111111111111111111111111111111"
        "1111111111111111111222222222222222222222222222222222222211112"
    ),
    "adayolo_bottleneck256_fwd": (
        "111111111122222111111111111111111111111111111111111111111111111111111111111111111111111111111111111111111122222222"
    ),
    "adayolo_bottleneck_ws_fwd": (
        "111111111122222111111111111111111111111111111111111111111111111111111111111111111111111111111111111111111111122222222"
    ),
    "adayolo_conv_keep_fwd": (
        "111111111222222222222112122111111111111111111111111111111111111111111111111111111111111111111111111111111111111111111111"
        "111111111111111111111111111111111111111111111111111111111111111111111111111111111111111111111111111111111111111111111111"
        "111111111111111111111111111111111111111111111111111111111111111111111111111111111111111111111111111111111111111111111111"
        "111111111111111111111111111111111111111111111111112222222222222122222222222222222222222222222222221222222222222222222222"
        "222222222221222222222222222222222222222222221222222222222222222222222222222212222222222222222222222222222221222222222222"
        "222222222222222212222222222222222222222222222122222222222222222222222222122222222222222222222222222122222222222222222222"
        "222212222222222222222222222221222222222222222222222111111111111111111111111111111111111111111111112222222222222222222221"
        "1111111111111111111122222222222222222222222222222222222222"
    ),
    "adayolo_conv_splitk_workspace_bytes": (
        "000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000"
        "0000000000000000000000000000000000000000000000000000000"
    ),
    "adayolo_conv_splitk_fwd": (
        "111111111222222222211222221122111111111111111111111111111111111111111111111111111111111111111111111111111111111111111111"
        "111111111111111111111111111111111111111111111111111111111111111111111111111111111111111111111111111111111111111111111111"
        "111111111111111111111111111111111111111111111111111111111111111111111111111111122222222222222212221111111222222222222222"
        "122211111112222222222222122211111112222222222222122211111112222222222221221111111222222222221222111111122222222212211111"
        "112222222221221111111222222212221111111222222212221111111122111111111111112211111111111112222122211111112212221111111221"
        "22211111111222111111112221111111111111111122111111121111111"
    ),
    "adayolo_conv_dsilu_fwd": (
        "111111112222222222222122122222111111111111111111111111111111111111111111111111111111111111111111111111111111111111111111"
        "111111111111111111111111111111111111111111111111111111111111111111111111111111111111111111111111111111111111111111111111"
        "111111111111111111111111111111111111111111111111111111111111111111111111111111111111111111111111111111111111111111111111"
        "111111111111111111111111111111122222222222122122222222222222222222222222222222221221222222222222222222222222222222221221"
        "222222222222222222222222222222221221222222222222222222222222222222212212222222222222222222222222222221221222222222222222"
        "222222222222212212222222222222222222222222222122122222222222222222222222222122122222222222222222222222222122122222222222"
        "222222222222212212222222222222222222222221221222222222222222222222221221222222222222222222222221111111111111111111111111"
        "112222222222222222222222212222222222222222222222211111111111111111111111222222222222222222222222222222222222222222222222"
        "222222222222"
    ),
    "adayolo_conv_s2grad_fwd": (
        "111111111122222222222222211111111111111111111111111111111111111111111111111111111111111111111111111111111111111111111111"
        "111111111111111111111111111111111111111111111111111111111111111111111111111111111111111111111111111111111111111111111111"
        "111111111111111111111111111111111111111111111111111111111111111111111111111111111111111111111111111111111111111111111111"
        "111111111111111111111111111111111111111111111111111111111111111111111111111222222222222222222222222222222222222222222222"
        "222222222222222222222222222222222222222222222222222222222222222222222222222222222222222222222222222222222222222222222222"
        "222222222222222222222222222222222222222222222222222222222222222222222222222222222222222222222222222222222222222222222222"
        "22222222222222222222222222222222222222222222222222222222222222222222222222"
    ),
    "adayolo_stem_fwd": (
        "111111111122221111111111111111111111111111111111111111111111111111111111111111111111111111111111122222"
    ),
    "adayolo_stem_fwd_act": (
        "111111111122221111111111111111111111111111111111111111111111111111111111111111111111111111111111111111111111111111111112"
        "221121121111"
    ),
    "adayolo_stem_keep_fwd": (
        "111111111122221221111111111111111111111111111111111111111111111111111111111111111111111111111111111111111111111111111111"
        "11111111112221222122212212211"
    ),
    "adayolo_letterbox_pack": (
        "1111111122211111111111111111111111111111111111111111111111111111111121211"
    ),
    "adayolo_stem_down_fwd": (
        "111111112211111122222111111111111111111111111111111111111111111111111111111111111111111111111111111111111111111111111111"
        "11111111111111111111111111111111122222222222222222222221111111111111111111111111111111111111111222222222"
    ),
    "adayolo_silu_fwd": (
        "1111222222221111111111111111111111111111111111111222222222222222222222222"
    ),
    "adayolo_silu_bwd": (
        "1111222222222211111111111111111111111111111111111111111111112222222222222222222222222222222222222222"
    ),
    "adayolo_zero_insert2x": (
        "1111111222222221111111111111111111111111111111111111111111111111111111111111111111111111112222222222222222222222222"
    ),
    "adayolo_upsample2x_bwd": (
        "111112222221111111111111111111111111111111111111111222222222222"
    ),
    "adayolo_image_grad": (
        "11111111221111111111111111111111111111111111111111111"
    ),
    "adayolo_upsample2x": (
        "111111222221111111111111111111111111111111111111111111122222222"
    ),
    "adayolo_detect_decode": (
        "11111111222211111111111111111111111111111111111111111111111111111111111122222"
    ),
    "adayolo_nms": (
        "111111211111111111111111111111111111111111111111222"
    ),
    "chain": (
        "011101110111011101110111011102210221022102210221022102210221011101110221022102210221022101110221011101110111011101110111"
        "011101110111011101110111011101110111011101110111011101110111011101110111011101110111011101110111011101110111011101110111"
        "011101110111011101110111011101110111011101110111011101110111011101110111011101110111011101110111011101110111011101110111"
        "011101110111011101110111011101110111011101110111011101110111011101110111011101110111011101110111011101110111011101110111"
        "011101110111011101110111011101110111011101110111011101110111011101110111011101110111011101110111011101110111011101110111"
        "011101110111011101110111011101110111011102210221022102210221022102210221022102210221022102210221022102210221022102210221"
        "022102210221022102210221022102210221022102210221022102210221011101110221022102210221022102210221022102210221011101110221"
        "022102210221022102210221022102210221011101110221022102210221022102210221022102210221022102210221022102210221022102210221"
        "022102210221022102210221022102210221022102210221022102210221022101110111011101110111011101110111011101110111022102210221"
        "02210221011102210221022101110221022101110221"
    ),
}


def test_adayolo_rejections_match_the_recorded_codes():
    """Every malformed call of the table returns the code recorded in _REJECT_CODES — also when two things are wrong at once."""
    from adaptiveisp_amd.yolo import _lib
    L = _lib.load()
    assert set(_REJECT_CODES) == set(_ENTRIES) | {"chain"}
    for name, want in _REJECT_CODES.items():
        got = _reject_codes(L, name)
        assert len(got) == len(want), name
        diff = [i for i in range(len(want)) if got[i] != want[i]]
        assert not diff, f"{name}: case {diff[0]} returns '{got[diff[0]]}', recorded '{want[diff[0]]}' ({len(diff)} of {len(want)} differ)"
    assert L.adayolo_conv_chain_fwd(None, 2, _C, 0, None) == -1 and L.adayolo_conv_chain_status(None) == -1
    assert L.adayolo_conv_chain_poll(_C) == -1                   # never prepared


def _print_reject_codes():
    from adaptiveisp_amd.yolo import _lib
    L = _lib.load()
    print("_REJECT_CODES = {")
    for name in list(_ENTRIES) + ["chain"]:
        codes = _reject_codes(L, name)
        assert "?" not in codes, (name, codes.index("?"))        # a case that is not refused does not belong in the table
        print(f'    "{name}": (')
        for i in range(0, len(codes), 120):
            print(f'        "{codes[i:i + 120]}"')
        print("    ),")
    print("}")


if __name__ == "__main__":
    import sys
    sys.path.insert(0, ROOT)
    _print_reject_codes()
