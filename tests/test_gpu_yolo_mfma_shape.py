"""The two MFMA shapes of the ring kernels' k-loop (adayolo_set_mfma_shape: 32 = v_mfma_f32_32x32x16_bf16, 16 =
v_mfma_f32_16x16x32_bf16; family 0 = the 256 px x 256 ch kernel, variant 50, family 1 = the 256 px x 128 ch kernel, variant 60,
with its split-K and keep forms; the chain kernel runs each tile type on its family's shape). Every case runs under both
shapes and restores the setting.

Bounds (none of them taken from what the kernels give):
  * against fp32 `F.conv2d` on the same bf16 operands (Conv.forward_fuse / Bottleneck.forward, yolov3/models/common.py:45-59,
    110-120): the project's bound for every conv variant (test_gpu_yolo_variants._check) — max |err| <= 2e-2 * max(1, max |ref|),
    mean |err| <= 2e-3 * that scale, NaN-prefilled outputs fully written, four launches bit-identical;
  * 16 against 32 on the same call: <= 2^-6 * scale — the two shapes add the same products in a different order inside a
    k-tile, so the results are two bf16 roundings (2^-8 relative each) of the same sum; the bound test_fused_3x3_plus_1x1 uses
    for that situation;
  * bit-exact under shape 16, as under 32: the fused pair's `out` against the unfused kernel, conv_keep against conv + silu_fwd,
    split-K over repeated launches on one workspace, a chain against its launch-per-layer run."""
import contextlib
import ctypes

import pytest
import torch

from _margins import close, close_scaled
from test_gpu_yolo_chain import _Net, _Net512
from test_gpu_yolo_variants import DEV, SPLITK_BASE, _reference, _run_variant, _splitk_bytes

pytestmark = pytest.mark.gpu
PP, PP128 = 0, 1
FAMILY = {50: PP, 60: PP128}


@contextlib.contextmanager
def mfma_shape(pp=None, pp128=None):
    from adaptiveisp_amd.yolo import _lib
    L = _lib.load()
    old = (L.adayolo_get_mfma_shape(PP), L.adayolo_get_mfma_shape(PP128))
    try:
        for fam, s in ((PP, pp), (PP128, pp128)):
            if s is not None:
                assert L.adayolo_set_mfma_shape(fam, s) == 0 and L.adayolo_get_mfma_shape(fam) == s
        yield
    finally:
        L.adayolo_set_mfma_shape(PP, old[0])
        L.adayolo_set_mfma_shape(PP128, old[1])


def test_setter_checks_its_arguments():
    from adaptiveisp_amd.yolo import _lib
    L = _lib.load()
    before = (L.adayolo_get_mfma_shape(PP), L.adayolo_get_mfma_shape(PP128))
    assert set(before) <= {16, 32}
    assert L.adayolo_set_mfma_shape(2, 16) == -1 and L.adayolo_set_mfma_shape(-1, 32) == -1
    assert L.adayolo_set_mfma_shape(PP, 8) == -1 and L.adayolo_set_mfma_shape(PP128, 0) == -1
    assert L.adayolo_get_mfma_shape(2) == -1
    assert (L.adayolo_get_mfma_shape(PP), L.adayolo_get_mfma_shape(PP128)) == before      # a refused call changes nothing
    with mfma_shape(16, 32):
        assert (L.adayolo_get_mfma_shape(PP), L.adayolo_get_mfma_shape(PP128)) == (16, 32)
    assert (L.adayolo_get_mfma_shape(PP), L.adayolo_get_mfma_shape(PP128)) == before


def _operands(shape, use_res, seed):
    B, H, W, cin, cout, k, s = shape
    g = torch.Generator(device="cpu").manual_seed(seed)
    x = torch.randn(B, H, W, cin, generator=g).to(torch.bfloat16).to(DEV)
    w = (torch.randn(cout, k, k, cin, generator=g) / (k * k * cin) ** 0.5).to(torch.bfloat16).to(DEV)
    b = torch.randn(cout, generator=g).to(DEV)
    Ho, Wo = (H - 1) // s + 1, (W - 1) // s + 1
    res = torch.randn(B, Ho, Wo, cout, generator=g).to(torch.bfloat16).to(DEV) if use_res else None
    return x, w, b, res


def _vs_fp32(tag, out, ref):
    assert torch.isfinite(out.float()).all(), f"{tag}: unwritten (NaN) outputs"
    scale = max(1.0, ref.abs().max().item())
    d = (out.float() - ref).abs()
    print(f"{tag}: max err {d.max().item():.3e} mean err {d.mean().item():.3e} scale {scale:.3f}")
    close_scaled("yolo.mfma_shape_vs_fp32", out.float(), ref, 2e-2, err_msg=tag)
    assert d.mean().item() <= 2e-3 * scale, f"{tag}: mean err {d.mean().item()}"
    return scale


# B, H, W, Cin, Cout, k, s, residual. k-tiles nK = k * k * Cin / 64; a 16-row fragment is partial when M % 16 != 0.
CASES = [
    (1, 1, 1, 64, 256, 3, 1, False),        # one pixel; nK = 9 (odd)
    (1, 5, 6, 512, 1024, 3, 1, True),       # M = 30: partial fragment, partial M tile, residual; 4 / 8 n-tiles
    (3, 9, 11, 64, 256, 1, 1, False),       # nK = 1; M = 297: two M tiles, the second partial
    (1, 9, 7, 192, 512, 3, 1, True),        # nK = 27 (odd); two n-tiles of 256 / four of 128
    (1, 7, 9, 64, 256, 3, 2, False),        # stride 2 on odd sizes; two n-tiles of 128
    (2, 19, 33, 128, 256, 3, 1, True),      # five M tiles, nK = 18, residual
    (1, 9, 7, 192, 384, 3, 1, True),        # 256 x 128 kernel only: three n-tiles, nK = 27
]


@pytest.mark.parametrize("case,v", [(c, v) for c in CASES for v in (50, 60) if v == 60 or c[4] % 256 == 0],
                         ids=lambda p: "x".join(map(str, p)) if isinstance(p, tuple) else f"v{p}")
def test_both_shapes_against_fp32_and_each_other(case, v):
    *shape, use_res = case
    B, H, W, cin, cout, k, s = shape
    x, w, b, res = _operands(shape, use_res, seed=H * 131 + cin * 7 + cout + v)
    for act in (0, 1):
        ref = _reference(x, w, b, res, k, s, act)
        outs = {}
        for ms in (32, 16):
            with mfma_shape(**{"pp" if v == 50 else "pp128": ms}):
                outs[ms] = _run_variant(x, w, b, res, k, s, act, v)          # four launches, bit-identical
            scale = _vs_fp32(f"{shape} v{v} act{act} shape {ms}", outs[ms], ref)
        d = (outs[16].float() - outs[32].float()).abs().max().item()
        print(f"{shape} v{v} act{act}: 16 vs 32 max diff {d:.3e} (bound {2.0 ** -6 * scale:.3e})")
        assert d <= 2.0 ** -6 * scale, f"{shape} v{v} act{act}: shapes differ by {d}"


@pytest.mark.parametrize("v", [50, 60])
@pytest.mark.parametrize("ms", [32, 16])
def test_channel_slices(v, ms):
    """Channel-sliced input, output and residual strides (test_gpu_yolo_variants.test_variant_channel_slices) under each shape."""
    from adaptiveisp_amd.yolo import _lib
    L = _lib.load()
    cin, cout, k, s = (64, 256, 3, 1)
    g = torch.Generator(device="cpu").manual_seed(50 + v)
    wide_in = torch.randn(2, 21, 35, cin + 64, generator=g).to(torch.bfloat16).to(DEV)
    wide_out = torch.full((2, 21, 35, cout + 128), 7.0, dtype=torch.bfloat16, device=DEV)
    wide_res = torch.randn(2, 21, 35, cout + 8, generator=g).to(torch.bfloat16).to(DEV)
    w = (torch.randn(cout, k, k, cin, generator=g) / 24).to(torch.bfloat16).to(DEV)
    b = torch.randn(cout, generator=g).to(DEV)
    xin, xout, xres = wide_in[..., 32:32 + cin], wide_out[..., 64:64 + cout], wide_res[..., 8:]
    with mfma_shape(**{"pp" if v == 50 else "pp128": ms}):
        rc = L.adayolo_conv_fwd_variant(ctypes.c_void_p(xin.data_ptr()), wide_in.shape[3], ctypes.c_void_p(w.data_ptr()),
                                        ctypes.c_void_p(b.data_ptr()), ctypes.c_void_p(xres.data_ptr()), wide_res.shape[3],
                                        ctypes.c_void_p(xout.data_ptr()), wide_out.shape[3], 2, 21, 35, cin, cout, k, s, 1, v,
                                        _lib.stream_ptr())
        _lib.check(rc, "conv")
        torch.cuda.synchronize()
    ref = _reference(xin.contiguous(), w, b, xres.contiguous(), k, s, 1)
    assert (xout.float() - ref).abs().max().item() <= 2e-2 * max(1.0, ref.abs().max().item())
    assert (wide_out[..., :64] == 7).all() and (wide_out[..., 64 + cout:] == 7).all()       # neighbours untouched


FUSED = [(2, 19, 33, 128, 3, 1, True), (1, 7, 9, 64, 3, 2, False), (1, 5, 6, 512, 3, 1, True)]   # B, H, W, Cin, k, s, residual


@pytest.mark.parametrize("ms", [32, 16])
@pytest.mark.parametrize("case", FUSED, ids=lambda c: "x".join(map(str, c)))
def test_fused_pair_first_layer_is_the_unfused_kernel(case, ms):
    """adayolo_conv_fused1x1_fwd: `out` bit-identical to variant 50 under the same shape; `out2` (the second GEMM stays on
    32x32x16 and its fragment-major weights) is the 1x1 conv of that bf16 output within the variants' bound."""
    from adaptiveisp_amd.yolo import _lib
    L = _lib.load()
    B, H, W, cin, k, s, use_res = case
    x, w, b, res = _operands((B, H, W, cin, 256, k, s), use_res, seed=H * 31 + cin)
    g = torch.Generator(device="cpu").manual_seed(cin + 1)
    w2 = (torch.randn(128, 1, 1, 256, generator=g) / 16.0).to(torch.bfloat16).to(DEV)
    b2 = torch.randn(128, generator=g).to(DEV)
    w2p = w2.reshape(4, 32, 16, 2, 8).permute(0, 2, 3, 1, 4).contiguous()
    Ho, Wo = (H - 1) // s + 1, (W - 1) // s + 1
    P = lambda t: ctypes.c_void_p(t.data_ptr()) if t is not None else None  # noqa: E731
    for act in (1, 0):                                   # the first layer's activation: SiLU (the engine's use), none
        with mfma_shape(pp=ms):
            first = None
            for _ in range(4):
                out = torch.full((B, Ho, Wo, 256), float("nan"), dtype=torch.bfloat16, device=DEV)
                out2 = torch.full((B, Ho, Wo, 128), float("nan"), dtype=torch.bfloat16, device=DEV)
                rc = L.adayolo_conv_fused1x1_fwd(P(x), cin, P(w), P(b), P(res), 256 if use_res else 0, P(out), 256, B, H, W, cin, 256,
                                                 k, s, act, P(w2p), P(b2), P(out2), 128, 128, _lib.stream_ptr())
                _lib.check(rc, "fused conv")
                torch.cuda.synchronize()
                if first is None:
                    first = (out, out2)
                else:
                    assert torch.equal(first[0].view(torch.int16), out.view(torch.int16)), "run-to-run difference (out)"
                    assert torch.equal(first[1].view(torch.int16), out2.view(torch.int16)), "run-to-run difference (out2)"
            out, out2 = first
            sep = _run_variant(x, w, b, res, k, s, act, 50, reps=1)
        assert torch.equal(sep.view(torch.int16), out.view(torch.int16)), "first layer differs from the unfused kernel"
        _vs_fp32(f"fused {case} shape {ms} act{act} out2", out2, _reference(out, w2, b2, None, 1, 1, 1))


@pytest.mark.parametrize("ms", [32, 16])
@pytest.mark.parametrize("case", [(2, 13, 17, 256, 128, 3, 1, True), (1, 5, 6, 512, 1024, 3, 1, False)],
                         ids=lambda c: "x".join(map(str, c)))
def test_keep_forward_is_conv_plus_silu(case, ms):
    """adayolo_conv_keep_fwd on the 256 x 128 kernel: `pre` is the act-none conv bit for bit, `out` is adayolo_silu_fwd of it."""
    from adaptiveisp_amd.yolo import _lib
    L = _lib.load()
    *shape, use_res = case
    B, H, W, cin, cout, k, s = shape
    x, w, b, res = _operands(shape, use_res, seed=cin + cout)
    with mfma_shape(pp128=ms):
        pre = torch.full((B, H, W, cout), float("nan"), dtype=torch.bfloat16, device=DEV)
        out = _run_variant(x, w, b, res, k, s, 1, 60, reps=2, pre=pre)
        lin = _run_variant(x, w, b, None, k, s, 0, 60, reps=1)
    assert torch.equal(pre.view(torch.int16), lin.view(torch.int16)), "pre is not the conv + bias output"
    two = torch.empty_like(out)
    rc = L.adayolo_silu_fwd(ctypes.c_void_p(pre.data_ptr()), cout, ctypes.c_void_p(res.data_ptr()) if use_res else None,
                            cout if use_res else 0, ctypes.c_void_p(two.data_ptr()), cout, B * H * W, cout, _lib.stream_ptr())
    _lib.check(rc, "silu_fwd")
    torch.cuda.synchronize()
    assert torch.equal(two.view(torch.int16), out.view(torch.int16)), "out differs from silu_fwd(pre, residual)"
    _vs_fp32(f"keep {case} shape {ms}", out, _reference(x, w, b, res, k, s, 1))


@pytest.mark.parametrize("case", [(2, 13, 17, 256, 128, 3, 1, True), (1, 5, 6, 1024, 512, 3, 1, False)],
                         ids=lambda c: "x".join(map(str, c)))
def test_splitk_is_bit_stable_and_close_under_both_shapes(case):
    """Every split the library serves for the shape: 16 launches on ONE workspace bit-identical (writer and reducer agree on the
    accumulator layout, the partial sums are added in split order whoever arrives last), fp32 bound, 16 against 32."""
    *shape, use_res = case
    B, H, W, cin, cout, k, s = shape
    served = [v for v in range(SPLITK_BASE + 2, SPLITK_BASE + 17) if _splitk_bytes(v, B, H, W, cin, cout, k, s) > 0]
    assert served, f"no split serves {case}"
    x, w, b, res = _operands(shape, use_res, seed=H * 131 + cin * 7 + cout)
    ref = _reference(x, w, b, res, k, s, 1)
    for v in served:
        outs = {}
        for ms in (32, 16):
            with mfma_shape(pp128=ms):
                outs[ms] = _run_variant(x, w, b, res, k, s, 1, v, reps=16)
            scale = _vs_fp32(f"{shape} split v{v} shape {ms}", outs[ms], ref)
        assert (outs[16].float() - outs[32].float()).abs().max().item() <= 2.0 ** -6 * scale


@pytest.mark.parametrize("pp,pp128", [(16, 16), (16, 32), (32, 16)])
def test_chain_equals_its_separate_launches(pp, pp128):
    """The smallest nets of test_gpu_yolo_chain.py (256 x 256 tiles with fused pairs; the mixed 256 x 256 / 256 x 128 net): the
    chain uses each tile type's selected shape, so it is bit-identical to the launch-per-layer run under the same setting."""
    with mfma_shape(pp, pp128):
        # ... with SiLU layers (the engine's chains), and with act none: the chain's other four epilogue forms per tile type
        for net, act in ((_Net(1, 16, 16, 64, 2, seed=116), 1), (_Net512(1, 20, 24, 256, 1, seed=30), 1),
                         (_Net(1, 16, 16, 64, 2, seed=117), 0), (_Net512(1, 20, 24, 256, 1, seed=31), 0)):
            net.act = act
            net.poison()
            net.run_separately()
            torch.cuda.synchronize()
            want = [t.clone() for t in net.outputs()]
            assert all(torch.isfinite(t.float()).all() for t in want)
            run = net.chain()
            for rep in range(4):
                net.poison()
                run()
                torch.cuda.synchronize()
                assert run.status() == 0
                for i, (got, ref) in enumerate(zip(net.outputs(), want)):
                    assert torch.equal(got, ref), (type(net).__name__, rep, i)


_ENGINE_REF = {}


def _engine_reference(B, H, W):
    if not _ENGINE_REF:
        from _synth import synth_yolo_state_dict, test_image
        from adaptiveisp_amd.yolo import YoloEngine, yolov3
        m = yolov3().eval()
        m.load_state_dict(synth_yolo_state_dict(m))
        x = torch.from_numpy(test_image(B, H, W, seed=91, special=False)).to(DEV)
        probe = YoloEngine(m, B, H, W, device=DEV)
        boxed = torch.full((B, 3, probe.Hp, W), 114 / 255, device=DEV)
        boxed[:, :, probe.pad_top:probe.pad_top + H] = x
        with torch.no_grad():
            ref = m.to(DEV)(boxed)[0].clone()
        m.to("cpu")
        _ENGINE_REF.update(m=m, x=x, ref=ref)
    return _ENGINE_REF["m"], _ENGINE_REF["x"], _ENGINE_REF["ref"]


@pytest.mark.parametrize("ms", [32, 16])
def test_engine_on_the_ring_kernels_vs_fp32_module_tree(ms):
    """YoloEngine(1 x 96 x 160) with every layer the two ring kernels serve routed to them (variant 50 where it fits, else 60;
    pairs and chains fused as in the tuned plan) against the fp32 module tree: decoded prediction within rtol = atol = 2e-2,
    the tuned engine's bound (test_gpu_yolo_variants._tuned_engine_vs_module_tree)."""
    from adaptiveisp_amd.yolo import YoloEngine
    from adaptiveisp_amd.yolo import engine as E
    B, H, W = 1, 96, 160
    m, x, ref = _engine_reference(B, H, W)
    with mfma_shape(ms, ms):
        eng = YoloEngine(m, B, H, W, device=DEV)
        n = {50: 0, 60: 0}
        for plan in eng._plans():
            for kind, _, args in plan:
                if kind == "conv":
                    key = E._conv_shape(args).key
                    v = 50 if E.serves(50, key) else 60 if E.serves(60, key) else None
                    if v:
                        args[E.ARG_VARIANT] = v
                        n[v] += 1
        assert n[50] >= 8 and n[60] >= 8, n
        eng.fuse_pairs()
        pred = eng(x).clone()
        torch.cuda.synchronize()
    close(f"yolo.mfma_shape_engine_pred_{H}x{W}", pred, ref, rtol=2e-2, atol=2e-2, err_msg=f"shape {ms}")
