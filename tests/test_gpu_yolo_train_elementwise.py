"""The element-wise training kernels of the detector (csrc/yolo_train.hip: k_silu_fwd, k_silu_bwd, k_zero_insert,
k_upsample_bwd, k_image_grad) through the C-ABI against float64, element by element: bf16-exact inputs, the reference rounded
to bf16 where the kernel rounds, every tensor a channel slice (offset 8, stride != C) of a wider buffer whose neighbouring
channels hold a sentinel that must survive, C in {8, 24, 64, 1024}, ragged H and W, and one case per kernel with more than
8192 * 256 work items, so the grid-stride loop takes a second trip. The float64 reference runs on the device (ATen's float64
element-wise kernels, nothing of this project).

Bounds, with u = 2^-8 (one bf16 ulp: half for the kernel's rounding, half for a tie flipped by fp32 noise), e = 2^-23:
  fp32 value of silu(x) = x * rcp(1 + exp2(-x log2 e)): the product in the exponent is rounded at |x| log2(e) e / 2, which the
  exponential turns into a relative |x| e / 2 ... taken as |x| e; v_exp and v_rcp are 1 ulp each, the add and the product half
  an ulp each: 3 e; together (4 + |x|) e |silu|. A sigmoid below the smallest normal fp32 (x < -87.3) may be flushed to zero
  by v_rcp: 2^-126 |x| absolutely.
  silu_fwd            |got - ref| <= u |silu| + (4 + |x|) e |silu| + 2^-126 |x|      (+ u |silu + res| with a residual: the
                      second rounding; the fp32 add of two bf16 values is below e of it)
  silu_bwd, grad_pre  the same rule on g * (s + x s (1 - s)), the fp32 term on the sum of the ABSOLUTE terms (silu' crosses
                      zero at x = -1.278): u |ref| + (8 + |x|) e |g| (s + |x| s (1 - s)) + 2^-126 |g| (1 + |x|)
  silu_bwd, grad_res  accumulate 0: a bit copy; accumulate 1: u |ref| + 2 e (|g| + |old|)
  upsample2x_bwd      u |ref| + 2^-22 (sum of the five |terms|)   (four fp32 adds)
  zero_insert2x, image_grad  bit-exact."""
import ctypes

import pytest
import torch

import _margins

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
BF = torch.bfloat16
U, E = 2.0 ** -8, 2.0 ** -23
SENTINEL = 0x7FC5                                   # a bf16 NaN with a payload in every channel a kernel must not write
BIG_PIX = 1450 * 1450                               # C = 8: one work item per pixel, more than 8192 * 256 = 2 097 152
SHAPES = [(2, 5, 7, 8), (1, 3, 11, 24), (3, 9, 5, 64), (1, 7, 3, 1024)]          # B, H, W, C


def _p(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


def _lib():
    from adaptiveisp_amd.yolo import _lib
    return _lib.load(), _lib.stream_ptr, _lib.check


def _wide(shape, C, fill=None, g=None, scale=1.0, special=()):
    """A [..., C] channel slice at offset 8 of a [..., C + 16] buffer. fill=None: randn * scale values (bf16) in the slice, with
    `special` values planted; the neighbouring channels hold the sentinel either way."""
    buf = torch.full((*shape, C + 16), SENTINEL, dtype=torch.int16, device=DEV).view(BF)
    view = buf[..., 8:8 + C]
    if fill is None:
        x = (torch.randn(*shape, C, generator=g) * scale).to(BF)
        flat = x.view(-1)
        for k, v in enumerate(special):
            flat[k::max(1, flat.numel() // 7) + 1][:3] = v
        view.copy_(x.to(DEV))
    else:
        view.copy_(torch.full((*shape, C), fill, dtype=torch.int16, device=DEV).view(BF))
    return buf, view


def _fence_ok(buf, C):
    b = buf.view(torch.int16)
    return bool((b[..., :8] == SENTINEL).all()) and bool((b[..., 8 + C:] == SENTINEL).all())


def _bf(x64):
    return x64.float().to(BF)


def _bits(t):
    return t.contiguous().view(torch.int16)


def _check(label, got, ref, bound, refb):
    """got (bf16) within `bound` of the float64 ref, element by element; returns the share that is not bf16(ref) itself."""
    d = (got.double() - ref).abs()
    assert torch.isfinite(got.float()).all(), f"{label}: non-finite output"
    worst = float((d / bound.clamp(min=1e-300)).max()) if d.numel() else 0.0
    print(f"{label}: worst share of the bound {worst:.3f}")
    assert (d <= bound).all(), f"{label}: error uses {worst:.3g}x the bound at {int((d > bound).sum())} elements"
    return float((_bits(got) != _bits(refb)).double().mean())


SHARES = {}


def _note(kernel, share):
    SHARES.setdefault(kernel, []).append(share)


def _silu64(x):
    return x * torch.sigmoid(x)


def _silu_terms(x):
    s = torch.sigmoid(x)
    return s, s + x * s * (1 - s), s + x.abs() * s * (1 - s)


SPECIAL = (20.0, -20.0, 88.0, -88.0, 0.0)


def _shapes(big):
    return [(1, 1450, 1450, 8)] if big else SHAPES


@pytest.mark.parametrize("big", [False, True], ids=["small", "gridstride"])
@pytest.mark.parametrize("use_res", [False, True], ids=["plain", "residual"])
def test_silu_fwd(big, use_res):
    L, st, check = _lib()
    for (B, H, W, C) in _shapes(big):
        g = torch.Generator().manual_seed(C + H)
        pbuf, pre = _wide((B, H, W), C, g=g, scale=4.0, special=SPECIAL)
        rbuf, res = _wide((B, H, W), C, g=g, scale=2.0) if use_res else (None, None)
        obuf, out = _wide((B, H, W), C, fill=SENTINEL)
        npix = B * H * W
        assert not big or npix * (C // 8) > 8192 * 256
        check(L.adayolo_silu_fwd(_p(pre), C + 16, _p(res), C + 16 if use_res else 0, _p(out), C + 16, npix, C, st()), "silu_fwd")
        torch.cuda.synchronize()
        x = pre.double()
        y = _silu64(x)
        bound = U * y.abs() + (4 + x.abs()) * E * y.abs() + 2.0 ** -126 * x.abs()
        ref, refb = y, _bf(y)
        if use_res:
            ref = y + res.double()
            bound = bound + U * ref.abs()
            refb = _bf(refb.double() + res.double())
        _note("silu_fwd", _check(f"silu_fwd {B}x{H}x{W}x{C} res={use_res}", out, ref, bound, refb))
        assert _fence_ok(obuf, C) and _fence_ok(pbuf, C) and (rbuf is None or _fence_ok(rbuf, C))
        assert not (_bits(out) == SENTINEL).any()
        # the saturated inputs took part
        assert bool((x == 88).any()) and bool((x == -88).any()) and bool((x == -20).any())


@pytest.mark.parametrize("big", [False, True], ids=["small", "gridstride"])
@pytest.mark.parametrize("accumulate", [0, 1])
@pytest.mark.parametrize("ptrs", ["gp", "gres", "both"])
def test_silu_bwd(ptrs, accumulate, big):
    L, st, check = _lib()
    for (B, H, W, C) in _shapes(big):
        g = torch.Generator().manual_seed(C + H + 1)
        gybuf, gy = _wide((B, H, W), C, g=g, scale=1.0, special=(0.0, 300.0))
        pbuf, pre = _wide((B, H, W), C, g=g, scale=4.0, special=SPECIAL)
        gpbuf, gp = _wide((B, H, W), C, fill=SENTINEL)
        grbuf, gres = _wide((B, H, W), C, g=g, scale=1.0, special=(0.0, -300.0))
        old = gres.double()
        want_gp, want_gres = ptrs in ("gp", "both"), ptrs in ("gres", "both")
        npix = B * H * W
        check(L.adayolo_silu_bwd(_p(gy), C + 16, _p(pre), C + 16, _p(gp) if want_gp else None, C + 16 if want_gp else 0,
                                 _p(gres) if want_gres else None, C + 16 if want_gres else 0, accumulate, npix, C, st()), "silu_bwd")
        torch.cuda.synchronize()
        gd, x = gy.double(), pre.double()
        if want_gp:
            s, d, dabs = _silu_terms(x)
            ref = gd * d
            bound = U * ref.abs() + (8 + x.abs()) * E * gd.abs() * dabs + 2.0 ** -126 * gd.abs() * (1 + x.abs())
            _note("silu_bwd", _check(f"silu_bwd gp {B}x{H}x{W}x{C}", gp, ref, bound, _bf(ref)))
            assert not (_bits(gp) == SENTINEL).any()
        else:
            assert (_bits(gp) == SENTINEL).all()                                   # not asked for: not written
        if want_gres and accumulate:
            ref = gd + old
            _note("silu_bwd", _check(f"silu_bwd gres+= {B}x{H}x{W}x{C}", gres, ref, U * ref.abs() + 2 * E * (gd.abs() + old.abs()), _bf(ref)))
        elif want_gres:
            assert torch.equal(_bits(gres), _bits(gy))                             # a bit copy
        else:
            assert torch.equal(gres.double(), old)
        assert all(_fence_ok(b, C) for b in (gybuf, pbuf, gpbuf, grbuf))


@pytest.mark.parametrize("big", [False, True], ids=["small", "gridstride"])
@pytest.mark.parametrize("odd_h,odd_w", [(0, 0), (1, 0), (0, 1), (1, 1)])
def test_zero_insert2x(odd_h, odd_w, big):
    L, st, check = _lib()
    for (B, Ho, Wo, C) in ([(1, 725, 725, 8)] if big else SHAPES):
        H, W = 2 * Ho - odd_h, 2 * Wo - odd_w
        assert not big or B * H * W * (C // 8) > 8192 * 256
        g = torch.Generator().manual_seed(C + Ho + 2)
        xbuf, x = _wide((B, Ho, Wo), C, g=g, special=(0.0, -0.0))
        ubuf, u = _wide((B, H, W), C, fill=SENTINEL)
        check(L.adayolo_zero_insert2x(_p(x), C + 16, _p(u), C + 16, B, Ho, Wo, H, W, C, st()), "zero_insert2x")
        torch.cuda.synchronize()
        ref = torch.zeros((B, H, W, C), dtype=BF, device=DEV)
        ref[:, 0::2, 0::2] = x
        assert torch.equal(_bits(u), _bits(ref)), (B, Ho, Wo, C, H, W)             # bit-exact (the inserted zeros are +0)
        assert _fence_ok(ubuf, C) and _fence_ok(xbuf, C)


@pytest.mark.parametrize("big", [False, True], ids=["small", "gridstride"])
@pytest.mark.parametrize("accumulate", [0, 1])
def test_upsample2x_bwd(accumulate, big):
    L, st, check = _lib()
    for (B, H, W, C) in _shapes(big):
        g = torch.Generator().manual_seed(C + H + 3)
        gybuf, gy = _wide((B, 2 * H, 2 * W), C, g=g, scale=2.0, special=(0.0, 500.0, -500.0))
        gxbuf, gx = _wide((B, H, W), C, g=g, scale=2.0, special=(0.0, 1000.0))
        old = gx.double() if accumulate else torch.zeros((B, H, W, C), dtype=torch.float64, device=DEV)
        assert not big or B * H * W * (C // 8) > 8192 * 256
        check(L.adayolo_upsample2x_bwd(_p(gy), C + 16, _p(gx), C + 16, accumulate, B, H, W, C, st()), "upsample2x_bwd")
        torch.cuda.synchronize()
        t = gy.double().view(B, H, 2, W, 2, C)
        ref = t.sum((2, 4)) + old
        mass = t.abs().sum((2, 4)) + old.abs()
        _note("upsample2x_bwd", _check(f"upsample2x_bwd {B}x{H}x{W}x{C} acc={accumulate}", gx, ref, U * ref.abs() + 2.0 ** -22 * mass,
                                       _bf(ref)))
        assert _fence_ok(gxbuf, C) and _fence_ok(gybuf, C)
        if accumulate:                                                          # the old content took part
            assert float((ref - t.sum((2, 4))).abs().max()) > 0


@pytest.mark.parametrize("B,H,W", [(2, 5, 7), (1, 33, 18), (3, 1000, 800)], ids=["5x7", "33x18", "gridstride"])
@pytest.mark.parametrize("g_cs", [8, 32])
@pytest.mark.parametrize("pad_top", [0, 12])
def test_image_grad(pad_top, g_cs, B, H, W):
    L, st, check = _lib()
    Hp = H + pad_top + (20 if pad_top else 0)                                   # letterbox rows above and below
    if (B, H, W) == (3, 1000, 800):
        assert B * H * W > 8192 * 256
    g = torch.Generator().manual_seed(H + g_cs)
    src = torch.randn(B, Hp, W, g_cs, generator=g).to(BF).to(DEV)
    src[:, :pad_top] = 777.0                                                    # what the letterbox rows hold must not appear
    src[:, pad_top + H:] = 777.0
    src[..., 3:] = 555.0                                                        # nor the other channels
    out = torch.full((B * 3 * H * W + 64,), float("nan"), device=DEV)           # 64 floats behind the image stay untouched
    check(L.adayolo_image_grad(_p(src), g_cs, _p(out), B, H, W, Hp, pad_top, st()), "image_grad")
    torch.cuda.synchronize()
    img = out[: B * 3 * H * W].view(B, 3, H, W)
    ref = src[:, pad_top:pad_top + H, :, :3].permute(0, 3, 1, 2).float()
    assert torch.equal(img.view(torch.int32), ref.contiguous().view(torch.int32))
    assert not (img == 777.0).any() and not (img == 555.0).any()
    assert torch.isnan(out[B * 3 * H * W:]).all()


def test_one_ulp_shares_are_recorded():
    """Runs last in the file: the share of elements that are not bf16(float64 reference) itself (one ulp away, within the
    bounds above), per kernel, for the parity-margins file. A measurement: expected to be a fraction of a per cent."""
    assert set(SHARES) >= {"silu_fwd", "silu_bwd", "upsample2x_bwd"}, "run the whole file"
    for k in sorted(SHARES):
        v = SHARES[k]
        line = f"yolo_train elementwise {k}: one-ulp share mean {sum(v) / len(v):.5%}, max {max(v):.5%} over {len(v)} tensors"
        print(line)
        _margins.NOTES.append(line)
