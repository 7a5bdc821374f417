"""ctypes binding of csrc/libadaisp.so — the C-ABI declared in include/adaisp.h.

PyTorch is plumbing here: it owns device memory and the HIP stream; every image operation below is a
kernel from the shared library. Nothing in this module falls back to eager PyTorch or to the CPU.
"""
import ctypes
import os

import numpy as np
import torch

_HERE = os.path.dirname(os.path.abspath(__file__))
# ADAISP_LIB: another BUILD of the same library (tools/build_variant.py); never a fallback
LIB_PATH = os.environ.get("ADAISP_LIB") or os.path.join(_HERE, "csrc", "libadaisp.so")

OP_ZERO, OP_EXPOSURE, OP_GAMMA, OP_CCM, OP_SHARPEN, OP_NLM, OP_TONE = -1, 0, 1, 2, 3, 4, 5
OP_CONTRAST, OP_SATPLUS, OP_WNB, OP_WB, OP_USM, OP_SHARPEN_V2, OP_COLOR = 6, 7, 8, 9, 10, 11, 12
MAX_PARAMS = 24
CLIP01 = 1
NLM_EXACT = 2      # NLM patch sums in the reference's running-sum order (slower); default is the separable kernel
NLM_SEP_V1 = 4     # the compiler-scheduled form of the separable kernel (cross-check / measurement)
NO_USM = 8         # adaisp_forward: no image selects the unsharp mask (its empty launch is skipped)
NLM_TILE32 = 16    # the 32-row tile of the default NLM kernel (cross-check / measurement)
ABI_VERSION = 9
UNP_UNPROCESS = 1  # adaisp_unprocess: the unprocess_wo_mosaic chain (default: convert, u8 / 255)
UNP_NOISE = 2      # adaisp_unprocess: + shot / read noise (needs UNP_UNPROCESS)

EXPORTS = ("adaisp_forward", "adaisp_forward_uniform", "adaisp_process", "adaisp_backward_params", "adaisp_backward_image", "adaisp_backward_image_workspace_bytes", "adaisp_pool64", "adaisp_pool64_backward", "adaisp_demosaic", "adaisp_unprocess", "adaisp_unprocess_bayer", "adaisp_demosaic_rects", "adaisp_demosaic_ex", "adaisp_demosaic_rects_ex", "adaisp_resize_u8", "adaisp_augment_u8", "adaisp_mosaic_u8", "adaisp_raw_load", "adaisp_raw_correct", "adaisp_export_u8", "adaisp_nlm_general", "adaisp_nlm_general_workspace_bytes", "adaisp_num_params",
           "adaisp_policy_conv", "adaisp_policy_fc1", "adaisp_policy_finish",
           "adaisp_trunk_train_fwd", "adaisp_trunk_train_bwd", "adaisp_trunk_train_workspace_bytes", "adaisp_trunk_train_scratch_bytes",
           "adaisp_critic_planes_fwd", "adaisp_critic_planes_bwd", "adaisp_td_fwd", "adaisp_td_bwd",
           "adaisp_policy_tail_fwd", "adaisp_policy_tail_bwd", "adaisp_image_stats", "adaisp_clip_adam_step", "adaisp_clip_adam_step_dev", "adaisp_heads_fwd", "adaisp_heads_bwd",
           "adaisp_strerror", "adaisp_abi_version")

_lib = None


class AdaispError(RuntimeError):
    pass


def load():
    """Load libadaisp.so (once). Raises — never degrades — if the library is absent or stale."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise AdaispError(f"{LIB_PATH} not found: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
                          "(hipcc --offload-arch=gfx950). There is no CPU/eager fallback for the ISP path.")
    L = ctypes.CDLL(LIB_PATH)
    vp, ci, cu = ctypes.c_void_p, ctypes.c_int, ctypes.c_uint
    L.adaisp_forward.argtypes = [vp, vp, vp, vp, vp, ci, ci, ci, ci, cu, vp]
    L.adaisp_forward_uniform.argtypes = [ci, vp, vp, vp, vp, ci, ci, ci, ci, cu, vp]
    L.adaisp_forward_uniform.restype = ci
    L.adaisp_process.argtypes = [ci, vp, vp, vp, ci, ci, ci, ci, cu, vp]
    L.adaisp_backward_params.argtypes = [vp, vp, vp, vp, ci, vp, ci, ci, ci, cu, vp]
    L.adaisp_backward_image.argtypes = [vp, vp, vp, vp, ci, vp, vp, ctypes.c_size_t, ci, ci, ci, cu, vp]
    L.adaisp_backward_image.restype = ci
    L.adaisp_backward_image_workspace_bytes.argtypes = [ci, ci, ci]
    L.adaisp_backward_image_workspace_bytes.restype = ctypes.c_size_t
    L.adaisp_pool64.argtypes = [vp, vp, ci, ci, ci, vp]
    L.adaisp_pool64_backward.argtypes = [vp, vp, ci, ci, ci, vp]
    L.adaisp_pool64_backward.restype = ci
    L.adaisp_demosaic.argtypes = [vp, vp, ci, ci, ci, ci, ctypes.c_float, ctypes.c_float, vp]
    L.adaisp_demosaic.restype = ci
    L.adaisp_unprocess.argtypes = [vp, vp, vp, ci, ci, ctypes.c_uint64, cu, vp]
    L.adaisp_unprocess.restype = ci
    L.adaisp_unprocess_bayer.argtypes = [vp, vp, vp, ci, ci, ctypes.c_uint64, cu, ci, ctypes.c_float, ctypes.c_float, vp]
    L.adaisp_unprocess_bayer.restype = ci
    L.adaisp_demosaic_rects.argtypes = [vp, vp, vp, ci, ci, ci, ctypes.c_float, ctypes.c_float, vp]
    L.adaisp_demosaic_rects.restype = ci
    L.adaisp_demosaic_ex.argtypes = [vp, vp, ci, ci, ci, ci, ci, ctypes.c_float, ctypes.c_float, vp]
    L.adaisp_demosaic_ex.restype = ci
    L.adaisp_demosaic_rects_ex.argtypes = [vp, vp, vp, ci, ci, ci, ci, ctypes.c_float, ctypes.c_float, vp]
    L.adaisp_demosaic_rects_ex.restype = ci
    sz = ctypes.c_size_t
    L.adaisp_resize_u8.argtypes = [vp, sz, vp, sz, vp, vp, sz, ci, ci, ci, vp]
    L.adaisp_resize_u8.restype = ci
    L.adaisp_augment_u8.argtypes = [vp, sz, vp, vp, ci, vp, ci, ci, cu, vp]
    L.adaisp_augment_u8.restype = ci
    L.adaisp_mosaic_u8.argtypes = [vp, sz, vp, vp, ci, vp, ci, ci, ci, vp]
    L.adaisp_mosaic_u8.restype = ci
    L.adaisp_raw_load.argtypes = [vp, sz, vp, vp, sz, vp, ci, ci, ci, ci, ctypes.c_float, ctypes.c_float, vp]
    L.adaisp_raw_load.restype = ci
    L.adaisp_raw_correct.argtypes = [vp, sz, vp, sz, vp, vp, sz, ci, vp]
    L.adaisp_raw_correct.restype = ci
    L.adaisp_export_u8.argtypes = [vp, vp, ci, ci, ci, vp]
    L.adaisp_export_u8.restype = ci
    L.adaisp_nlm_general.argtypes = [vp, vp, vp, ci, vp, ctypes.c_size_t, ci, ci, ci, ci, ci, vp]
    L.adaisp_nlm_general.restype = ci
    L.adaisp_nlm_general_workspace_bytes.argtypes = [ci, ci, ci]
    L.adaisp_nlm_general_workspace_bytes.restype = ctypes.c_size_t
    for name in ("adaisp_trunk_train_fwd", "adaisp_trunk_train_bwd", "adaisp_critic_planes_fwd", "adaisp_critic_planes_bwd",
                 "adaisp_td_fwd", "adaisp_td_bwd", "adaisp_policy_tail_fwd", "adaisp_policy_tail_bwd", "adaisp_heads_fwd", "adaisp_heads_bwd"):
        getattr(L, name).argtypes = [vp, vp]
        getattr(L, name).restype = ci
    for name in ("adaisp_trunk_train_workspace_bytes", "adaisp_trunk_train_scratch_bytes"):
        getattr(L, name).argtypes = [vp]
        getattr(L, name).restype = ctypes.c_size_t
    L.adaisp_image_stats.argtypes = [vp, vp, vp, ci, ctypes.c_long, vp]
    L.adaisp_clip_adam_step.argtypes = [vp, ci, ctypes.c_long, vp, ctypes.c_float] + [ctypes.c_double] * 4 + [vp]
    L.adaisp_clip_adam_step.restype = ci
    L.adaisp_clip_adam_step_dev.argtypes = [vp, ci, ctypes.c_long, vp, ctypes.c_float, vp] + [ctypes.c_double] * 3 + [vp]
    L.adaisp_clip_adam_step_dev.restype = ci
    L.adaisp_image_stats.restype = ci
    L.adaisp_num_params.argtypes = [ci]
    L.adaisp_strerror.argtypes = [ci]
    L.adaisp_strerror.restype = ctypes.c_char_p
    for name in ("adaisp_forward", "adaisp_process", "adaisp_backward_params", "adaisp_backward_image", "adaisp_backward_image_workspace_bytes", "adaisp_pool64", "adaisp_num_params",
                 "adaisp_abi_version"):
        getattr(L, name).restype = ci
    if L.adaisp_abi_version() != ABI_VERSION:
        raise AdaispError(f"libadaisp.so ABI {L.adaisp_abi_version()} != expected {ABI_VERSION}: rebuild")
    _lib = L
    return L


def _check(rc, what):
    if rc != 0:
        raise AdaispError(f"{what} failed: {load().adaisp_strerror(rc).decode()} ({rc})")


def _dev_f32(t, name):
    if not isinstance(t, torch.Tensor):
        raise TypeError(f"{name} must be a torch.Tensor")
    if not t.is_cuda:
        raise AdaispError(f"{name} is on {t.device}: the ISP kernels run on the HIP device only (no CPU fallback)")
    if t.dtype != torch.float32:
        raise TypeError(f"{name} must be float32, got {t.dtype}")
    return t.contiguous()


def _wrote(t):
    """A kernel wrote `t` through its raw pointer: tell torch (version counter), so that anything keyed on the tensor's
    version — autograd's saved-tensor checks, Agent's cached pooling of its last output — sees the change."""
    if t is not None:
        torch.autograd.graph.increment_version(t)


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _img_shape(img):
    if img.dim() != 4 or img.shape[1] != 3:
        raise ValueError(f"expected a [B,3,H,W] image, got {tuple(img.shape)}")
    return int(img.shape[0]), int(img.shape[2]), int(img.shape[3])


def image_stats(img):
    """[B,2] = (mean, number of non-finite values) per image of a [B,...] fp32 batch (adaisp_image_stats)."""
    L = load()
    img = _dev_f32(img.detach(), "img")
    B = int(img.shape[0])
    buf = torch.empty((B, 2 + 128), dtype=torch.float32, device=img.device)
    with torch.cuda.device(img.device):
        rc = L.adaisp_image_stats(img.data_ptr(), buf.data_ptr(), buf.data_ptr() + 8 * B, B, img.numel() // B, _stream())
    _check(rc, "adaisp_image_stats")
    return buf.view(-1)[:2 * B].view(B, 2)


def process(op, img, params, clip=False, out=None, nlm_exact=False, nlm_v1=False, nlm_tile32=False):
    """adaisp_process: one host-known op for the whole batch. params [B,n] (regressed)."""
    L = load()
    img = _dev_f32(img, "img")
    B, H, W = _img_shape(img)
    params = _dev_f32(params.reshape(B, -1), "params")
    if out is None:
        out = torch.empty_like(img)
    with torch.cuda.device(img.device):
        rc = L.adaisp_process(int(op), img.data_ptr(), out.data_ptr(), params.data_ptr(), params.shape[1], B, H, W,
                              (CLIP01 if clip else 0) | (NLM_EXACT if nlm_exact else 0) | (NLM_SEP_V1 if nlm_v1 else 0) |
                              (NLM_TILE32 if nlm_tile32 else 0),
                              _stream())
    _check(rc, "adaisp_process")
    _wrote(out)
    return out


def forward(img, op_ids, params, clip=True, pooled=None, out=None, nlm_exact=False, no_usm=False, host_op=None):
    """adaisp_forward: image b is filtered by op_ids[b] (int32, device). params [B,stride]. `pooled` ([B,3,64,64]) receives
    the 64x64 pooling of the result (fused into the filter launch where the geometry allows). `host_op`: the caller KNOWS
    that every op_ids[b] == host_op (a teacher-forced step) -> adaisp_forward_uniform, one launch instead of one per family."""
    L = load()
    img = _dev_f32(img, "img")
    B, H, W = _img_shape(img)
    params = _dev_f32(params.reshape(B, -1), "params")
    if host_op is None:
        if op_ids.dtype != torch.int32 or not op_ids.is_cuda:
            raise TypeError("op_ids must be an int32 device tensor")
        op_ids = op_ids.contiguous()
    if pooled is not None and (tuple(pooled.shape) != (B, 3, 64, 64) or pooled.dtype != torch.float32 or
                               pooled.device != img.device or not pooled.is_contiguous()):
        raise ValueError(f"pooled must be a contiguous float32 [{B},3,64,64] tensor on {img.device}")
    if out is None:
        out = torch.empty_like(img)
    elif (out.shape != img.shape or out.dtype != torch.float32 or out.device != img.device or not out.is_contiguous()):
        raise ValueError(f"out must be a contiguous float32 {tuple(img.shape)} tensor on {img.device}, got {out.dtype} "
                         f"{tuple(out.shape)} on {out.device}")
    flags = (CLIP01 if clip else 0) | (NLM_EXACT if nlm_exact else 0) | (NO_USM if no_usm else 0)
    with torch.cuda.device(img.device):
        if host_op is not None:
            rc = L.adaisp_forward_uniform(int(host_op), img.data_ptr(), out.data_ptr(),
                                          pooled.data_ptr() if pooled is not None else None, params.data_ptr(),
                                          params.shape[1], B, H, W, flags, _stream())
        else:
            rc = L.adaisp_forward(img.data_ptr(), out.data_ptr(), pooled.data_ptr() if pooled is not None else None,
                                  op_ids.data_ptr(), params.data_ptr(), params.shape[1], B, H, W, flags, _stream())
    _check(rc, "adaisp_forward")
    _wrote(out)
    _wrote(pooled)
    return out


def nlm_general(img, h, search_window_size, patch_size, out=None):
    """adaisp_nlm_general: NonLocalMeansGray(search_window_size, patch_size).forward(img, h) for any odd sizes (the ISP's
    11 / 5 goes through OP_NLM's tuned kernel). h: one value per image."""
    L = load()
    img = _dev_f32(img, "img")
    B, H, W = _img_shape(img)
    h = _dev_f32(h.reshape(B, -1), "h")
    if out is None:
        out = torch.empty_like(img)
    nbytes = int(L.adaisp_nlm_general_workspace_bytes(B, H, W))
    ws = torch.empty(nbytes // 4, dtype=torch.float32, device=img.device)
    with torch.cuda.device(img.device):
        rc = L.adaisp_nlm_general(img.data_ptr(), out.data_ptr(), h.data_ptr(), h.shape[1], ws.data_ptr(), nbytes, B, H, W,
                                  int(search_window_size), int(patch_size), _stream())
    _check(rc, "adaisp_nlm_general")
    _wrote(out)
    return out


def backward_params(img, grad_out, op_ids, params, clip=True):
    L = load()
    img = _dev_f32(img, "img")
    grad_out = _dev_f32(grad_out, "grad_out")
    B, H, W = _img_shape(img)
    params = _dev_f32(params.reshape(B, -1), "params")
    grad = torch.empty_like(params)
    with torch.cuda.device(img.device):
        rc = L.adaisp_backward_params(img.data_ptr(), grad_out.data_ptr(), op_ids.contiguous().data_ptr(),
                                      params.data_ptr(), params.shape[1], grad.data_ptr(), B, H, W,
                                      CLIP01 if clip else 0, _stream())
    _check(rc, "adaisp_backward_params")
    return grad


def backward_image(img, grad_out, op_ids, params, clip=True):
    """adaisp_backward_image: d/d img of sum(grad_out * adaisp_forward(img, op_ids, params, clip)) -> [B,3,H,W].
    op_ids int32 [B] on the device; the workspace comes from the torch allocator (capturable in a CUDA graph)."""
    L = load()
    img = _dev_f32(img, "img")
    grad_out = _dev_f32(grad_out, "grad_out")
    B, H, W = _img_shape(img)
    if tuple(grad_out.shape) != tuple(img.shape):
        raise ValueError(f"grad_out {tuple(grad_out.shape)} does not match img {tuple(img.shape)}")
    if op_ids.dtype != torch.int32 or not op_ids.is_cuda or op_ids.numel() != B:
        raise TypeError(f"op_ids must be an int32 device tensor of {B} ids")
    params = _dev_f32(params.reshape(B, -1), "params")
    grad = torch.empty_like(img)
    nbytes = int(L.adaisp_backward_image_workspace_bytes(B, H, W))
    ws = torch.empty(nbytes // 4, dtype=torch.float32, device=img.device)
    with torch.cuda.device(img.device):
        rc = L.adaisp_backward_image(img.data_ptr(), grad_out.data_ptr(), op_ids.contiguous().data_ptr(), params.data_ptr(),
                                     params.shape[1], grad.data_ptr(), ws.data_ptr(), nbytes, B, H, W,
                                     CLIP01 if clip else 0, _stream())
    _check(rc, "adaisp_backward_image")
    return grad


def pool64(img):
    """AdaptiveAvgPool2d((64,64)) of a [B,3,H,W] device image."""
    L = load()
    img = _dev_f32(img, "img")
    B, H, W = _img_shape(img)
    out = torch.empty((B, 3, 64, 64), dtype=torch.float32, device=img.device)
    with torch.cuda.device(img.device):
        rc = L.adaisp_pool64(img.data_ptr(), out.data_ptr(), B, H, W, _stream())
    _check(rc, "adaisp_pool64")
    return out


def pool64_backward(grad_pooled, H, W):
    """grad_pooled [B,3,64,64] -> gradient w.r.t. the [B,3,H,W] image that adaisp_pool64 pooled."""
    L = load()
    g = _dev_f32(grad_pooled, "grad_pooled")
    B = g.shape[0]
    if tuple(g.shape[1:]) != (3, 64, 64):
        raise AdaispError(f"grad_pooled must be [B,3,64,64], got {tuple(g.shape)}")
    out = torch.empty((B, 3, H, W), dtype=torch.float32, device=g.device)
    with torch.cuda.device(g.device):
        rc = L.adaisp_pool64_backward(g.data_ptr(), out.data_ptr(), B, H, W, _stream())
    _check(rc, "adaisp_pool64_backward")
    return out


CFA = {"RGGB": 0, "GRBG": 1, "GBRG": 2, "BGGR": 3}
DEMOSAIC = {"bilinear": 0, "mhc": 1}    # ADAISP_DEMOSAIC_*: 3 x 3 bilinear; 5 x 5 gradient-corrected (Malvar-He-Cutler)
U16 = (torch.uint16, torch.int16)       # the same 16 bits: torch's uint16 is young, int16 views carry planes as well


# ---- the front-end wrappers' argument checks (AdaispError naming the wrapper `what` and the argument, before any device work)
def _method(what, method):
    if not isinstance(method, str) or method not in DEMOSAIC:
        raise AdaispError(f"{what}: method must be one of {sorted(DEMOSAIC)}, got {method!r}")
    return DEMOSAIC[method]


def _pattern(pattern):
    return CFA[pattern.upper()] if isinstance(pattern, str) else int(pattern)


def _dtype_name(dtype):
    return str(dtype[0] if isinstance(dtype, tuple) else dtype).replace("torch.", "")


def _on_device(what, t, name, dtype=None):
    """`t` is a contiguous tensor on a HIP device, of `dtype` (one, or a tuple of equivalents) when given."""
    if not isinstance(t, torch.Tensor) or t.device.type != "cuda":
        raise AdaispError(f"{what}: {name} must be a HIP device tensor (there is no CPU path)")
    if not t.is_contiguous():
        raise AdaispError(f"{what}: {name} must be contiguous")
    if dtype is not None and t.dtype not in (dtype if isinstance(dtype, tuple) else (dtype,)):
        raise AdaispError(f"{what}: {name} must be a {_dtype_name(dtype)} tensor, got {t.dtype}")
    return t


def _records(what, desc, dtype):
    """The number of `dtype` records (a numpy record dtype) in the device byte tensor `desc`."""
    _on_device(what, desc, "desc", torch.uint8)
    if desc.numel() % dtype.itemsize:
        raise AdaispError(f"{what}: desc holds {desc.numel()} bytes, not a whole number of {dtype.itemsize}-byte records")
    return desc.numel() // dtype.itemsize


def _tab_words(what, tabs):
    """The number of int32 words in the device tensor `tabs`: an int32 tensor or 4-byte aligned bytes."""
    _on_device(what, tabs, "tabs")
    if tabs.dtype not in (torch.uint8, torch.int32) or tabs.data_ptr() % 4 or (tabs.numel() * tabs.element_size()) % 4:
        raise AdaispError(f"{what}: tabs must be int32 words (an int32 tensor or 4-byte aligned bytes)")
    return tabs.numel() * tabs.element_size() // 4


def _out(what, out, shape, dtype, device, alloc=None):
    """`out` if it is a contiguous `dtype` tensor of `shape` on `device`; a new one (of shape `alloc`, else `shape`) for None."""
    if out is None:
        return torch.empty(alloc or shape, dtype=dtype[0] if isinstance(dtype, tuple) else dtype, device=device)
    if (not isinstance(out, torch.Tensor) or tuple(out.shape) != tuple(shape) or not out.is_contiguous() or out.device != device
            or out.dtype not in (dtype if isinstance(dtype, tuple) else (dtype,))):
        raise AdaispError(f"{what}: out must be a contiguous {_dtype_name(dtype)} [{','.join(map(str, shape))}] tensor on the "
                          f"HIP device {device}")
    return out


def demosaic(raw, pattern="RGGB", black_level=0.0, white_level=65535.0, out=None, method="bilinear"):
    """Bayer front-end: raw uint16 [B,H,W] on the device -> planar fp32 [B,3,H,W] in [0,1] (include/adaisp.h); `method`
    "bilinear" or "mhc" (adaisp_demosaic_ex; "mhc" is not clamped and can leave [0,1] at edges)."""
    L, meth = load(), _method("demosaic", method)
    raw = _on_device("demosaic", raw.contiguous() if isinstance(raw, torch.Tensor) else raw, "raw")
    if raw.dtype not in U16 or raw.dim() != 3:
        raise AdaispError(f"demosaic: raw must be uint16 [B,H,W], got {raw.dtype} {tuple(raw.shape)}")
    B, H, W = raw.shape
    out = _out("demosaic", out, (B, 3, H, W), torch.float32, raw.device)
    with torch.cuda.device(raw.device):
        rc = L.adaisp_demosaic_ex(raw.data_ptr(), out.data_ptr(), B, H, W, _pattern(pattern), meth, float(black_level),
                                  float(white_level), _stream())
    _check(rc, "adaisp_demosaic_ex")
    _wrote(out)
    return out


# adaisp_unprocess_desc (include/adaisp.h): one 96-byte record per image
UNPROCESS_DESC = np.dtype([("src_offset", "<i8"), ("h", "<i4"), ("w", "<i4"), ("top", "<i4"), ("left", "<i4"),
                           ("serial", "<u8"), ("p", "<f4", (16,))], align=True)
assert UNPROCESS_DESC.itemsize == 96


def unprocess(src, desc, S, seed=0, flags=0, out=None):
    """adaisp_unprocess: uint8 HWC BGR images packed in the device byte tensor `src` (any offset: a slice is fine) ->
    planar fp32 [B,3,S,S], letterboxed by `desc` (B records of UNPROCESS_DESC as a device byte tensor). flags: 0 (u8 / 255),
    UNP_UNPROCESS, UNP_UNPROCESS | UNP_NOISE. Raises on bad arguments before any device work."""
    L = load()
    _on_device("unprocess", src, "src", torch.uint8)
    B, S = _records("unprocess", desc, UNPROCESS_DESC), int(S)
    out = _out("unprocess", out, (B, 3, S, S), torch.float32, src.device, alloc=(max(B, 1), 3, max(S, 1), max(S, 1)))
    with torch.cuda.device(src.device):
        rc = L.adaisp_unprocess(src.data_ptr(), desc.data_ptr(), out.data_ptr(), B, S, int(seed) & (2 ** 64 - 1),
                                int(flags), _stream())
    _check(rc, "adaisp_unprocess")
    _wrote(out)
    return out


def unprocess_bayer(src, desc, S, seed=0, flags=0, pattern="RGGB", black_level=0.0, white_level=65535.0, out=None):
    """adaisp_unprocess_bayer: `unprocess` seen through a colour filter array and quantised -> uint16 [B,S,S] on the
    device. src / desc / S / seed / flags as `unprocess`; a sample is the channel the CFA keeps at that pixel of the image
    (phase from the image's origin), clamp(rint(v * (white - black)) + black, 0, 65535), and `black` outside the image."""
    L = load()
    _on_device("unprocess_bayer", src, "src", torch.uint8)
    B, S = _records("unprocess_bayer", desc, UNPROCESS_DESC), int(S)
    out = _out("unprocess_bayer", out, (B, S, S), U16, src.device, alloc=(max(B, 1), max(S, 1), max(S, 1)))
    with torch.cuda.device(src.device):
        rc = L.adaisp_unprocess_bayer(src.data_ptr(), desc.data_ptr(), out.data_ptr(), B, S, int(seed) & (2 ** 64 - 1),
                                      int(flags), _pattern(pattern), float(black_level), float(white_level), _stream())
    _check(rc, "adaisp_unprocess_bayer")
    _wrote(out)
    return out


def demosaic_rects(raw, desc, pattern="RGGB", black_level=0.0, white_level=65535.0, out=None, method="bilinear"):
    """adaisp_demosaic_rects_ex: the letterboxed uint16 [B,S,S] plane of `unprocess_bayer` and its descriptors -> planar
    fp32 [B,3,S,S]: `demosaic` (same `method`) inside every image's own rectangle (phase and mirror at the rectangle),
    exactly 0 outside."""
    L, meth = load(), _method("demosaic_rects", method)
    _on_device("demosaic_rects", raw, "raw")
    B = _records("demosaic_rects", desc, UNPROCESS_DESC)
    if raw.dtype not in U16 or raw.dim() != 3 or raw.shape[1] != raw.shape[2]:
        raise AdaispError(f"demosaic_rects: raw must be a contiguous uint16 [B,S,S] tensor, got {raw.dtype} {tuple(raw.shape)}")
    if raw.shape[0] != B or raw.device != desc.device:
        raise AdaispError(f"demosaic_rects: {raw.shape[0]} planes on {raw.device} but {B} descriptors on {desc.device}")
    S = int(raw.shape[1])
    out = _out("demosaic_rects", out, (B, 3, S, S), torch.float32, raw.device)
    with torch.cuda.device(raw.device):
        rc = L.adaisp_demosaic_rects_ex(raw.data_ptr(), desc.data_ptr(), out.data_ptr(), B, S, _pattern(pattern), meth,
                                        float(black_level), float(white_level), _stream())
    _check(rc, "adaisp_demosaic_rects_ex")
    _wrote(out)
    return out


# adaisp_resize_desc (include/adaisp.h): one 56-byte record per image
RESIZE_DESC = np.dtype([("src_offset", "<i8"), ("dst_offset", "<i8"), ("tab_x", "<i8"), ("tab_y", "<i8"),
                        ("src_h", "<i4"), ("src_w", "<i4"), ("dst_h", "<i4"), ("dst_w", "<i4"), ("mode", "<i4"),
                        ("scale", "<f4")], align=True)
assert RESIZE_DESC.itemsize == 56
RESIZE_COPY, RESIZE_LINEAR, RESIZE_AREA_INT, RESIZE_AREA = 0, 1, 2, 3


def _check_resize_records(records, src_bytes, dst_bytes, tab_words):
    """What adaisp_resize_u8 would skip on the device is an error here: a mode, size or extent outside the buffers."""
    r = records
    if np.any((r["mode"] < RESIZE_COPY) | (r["mode"] > RESIZE_AREA)):
        raise AdaispError(f"resize_u8: unknown mode in {sorted(set(r['mode'].tolist()))}")
    for k in ("src_h", "src_w", "dst_h", "dst_w"):
        if np.any((r[k] < 1) | (r[k] > 32768)):
            raise AdaispError(f"resize_u8: {k} outside [1, 32768]")
    sb = r["src_h"].astype(np.int64) * r["src_w"] * 3
    db = r["dst_h"].astype(np.int64) * r["dst_w"] * 3
    if np.any(r["src_offset"] < 0) or np.any(r["src_offset"] + sb > src_bytes):
        raise AdaispError(f"resize_u8: a source image lies outside src ({src_bytes} bytes)")
    if np.any(r["dst_offset"] < 0) or np.any(r["dst_offset"] + db > dst_bytes):
        raise AdaispError(f"resize_u8: a destination image lies outside dst ({dst_bytes} bytes)")
    same = (r["src_h"] == r["dst_h"]) & (r["src_w"] == r["dst_w"])
    if np.any((r["mode"] == RESIZE_COPY) != same):
        raise AdaispError("resize_u8: COPY is the mode of equal sizes, and only of them")
    ai = r["mode"] == RESIZE_AREA_INT
    if np.any(ai & ((r["src_w"] % r["dst_w"] != 0) | (r["src_h"] % r["dst_h"] != 0))):
        raise AdaispError("resize_u8: AREA_INT needs integer factors")
    tabbed = (r["mode"] == RESIZE_LINEAR) | (r["mode"] == RESIZE_AREA)
    need = np.where(r["mode"] == RESIZE_LINEAR, 4, 1)           # LINEAR: 4 words per index; AREA: at least ptr[n + 1]
    ends = np.maximum(r["tab_x"] + need * r["dst_w"] + (r["mode"] == RESIZE_AREA),
                      r["tab_y"] + need * r["dst_h"] + (r["mode"] == RESIZE_AREA))
    if np.any(tabbed & ((r["tab_x"] < 0) | (r["tab_y"] < 0) | (ends > tab_words))):
        raise AdaispError(f"resize_u8: taps outside tabs ({tab_words} words)")


def resize_u8(src, dst, desc, tabs, records):
    """adaisp_resize_u8: uint8 HWC BGR images packed in the device byte tensor `src` -> `dst` (device bytes), image b
    resampled as records[b] says (RESIZE_DESC: sizes, mode, byte offsets into src / dst, word offsets of its taps in
    `tabs`). `desc` is the same records as a device byte tensor, `tabs` the taps (adaptiveisp_amd/resize.py) as a device
    int32 tensor or a 4-byte aligned byte tensor, or None when no image needs taps. `records` (host) sizes the launch and
    is checked against the buffers: raises on host tensors or malformed records before any device work. Capturable."""
    L = load()
    for t, name in ((src, "src"), (dst, "dst"), (desc, "desc")):
        _on_device("resize_u8", t, name, torch.uint8)
    tab_words = 0 if tabs is None else _tab_words("resize_u8", tabs)
    if not isinstance(records, np.ndarray) or records.dtype != RESIZE_DESC or records.ndim != 1 or len(records) < 1:
        raise AdaispError("resize_u8: records must be a non-empty 1-D numpy array of RESIZE_DESC")
    if desc.numel() != records.nbytes:
        raise AdaispError(f"resize_u8: desc holds {desc.numel()} bytes, records {records.nbytes}")
    _check_resize_records(records, src.numel(), dst.numel(), tab_words)
    B = len(records)
    with torch.cuda.device(src.device):
        rc = L.adaisp_resize_u8(src.data_ptr(), src.numel(), dst.data_ptr(), dst.numel(), desc.data_ptr(),
                                None if tabs is None else tabs.data_ptr(), tab_words, B, int(records["dst_h"].max()),
                                int(records["dst_w"].max()), _stream())
    _check(rc, "adaisp_resize_u8")
    _wrote(dst)
    return dst


# adaisp_augment_desc (include/adaisp.h): one 80-byte record per image
AUGMENT_DESC = np.dtype([("src_offset", "<i8"), ("h", "<i4"), ("w", "<i4"), ("top", "<i4"), ("left", "<i4"),
                         ("m", "<i8", (6,)), ("lut", "<i4"), ("reserved", "<i4")], align=True)
assert AUGMENT_DESC.itemsize == 80
AUGMENT_M_MAX = 2 ** 40          # |m| below it: with x, y < 2^15 the 64-bit sums cannot wrap


# ---- the rules augment and mosaic records share, on arrays of any shape; `live` masks the entries that count
def _rule_table(what, lut, n_luts):
    if np.any((lut < -1) | (lut >= n_luts)):
        raise AdaispError(f"{what}: a table index outside [-1, {n_luts})")


def _rule_map(what, m, live=True):
    if np.any(live & (np.abs(m) >= AUGMENT_M_MAX)):
        raise AdaispError(f"{what}: a map entry of 2^40 or more (Q16): the 64-bit sums could wrap")


def _rule_inside(what, whose, r, src_bytes, live=True):
    """The h * w * 3 bytes at src_offset of every record (or tile) `r` lie inside src."""
    nbytes = r["h"].astype(np.int64) * r["w"] * 3
    if np.any(live & ((r["src_offset"] < 0) | (r["src_offset"] + nbytes > src_bytes))):
        raise AdaispError(f"{what}: {whose} lies outside src ({src_bytes} bytes)")


def _check_augment_records(records, src_bytes, n_luts, S):
    """What adaisp_augment_u8 would turn into an all-fill image, or a map it would wrap, is an error here."""
    r = records
    if np.any((r["h"] < 0) | (r["w"] < 0) | (r["top"] < 0) | (r["left"] < 0) | (r["top"] > S - r["h"].astype(np.int64))
              | (r["left"] > S - r["w"].astype(np.int64))):
        raise AdaispError(f"augment_u8: an image's placement does not fit the {S} x {S} frame")
    _rule_inside("augment_u8", "a source image", r, src_bytes)
    _rule_table("augment_u8", r["lut"], n_luts)
    _rule_map("augment_u8", r["m"])


def _warp_u8(what, dtype, check, scalar, scalar_error, src, desc, luts, S, out, records):
    """augment_u8 and mosaic_u8: `dtype` records checked by `check(records, src_bytes, n_luts, S)`, the C entry
    adaisp_<what> with the trailing `scalar`, which is refused with `scalar_error` when that is not None."""
    L = load()
    _on_device(what, src, "src", torch.uint8)
    B, S = _records(what, desc, dtype), int(S)
    n_luts = 0
    if luts is not None:
        if _on_device(what, luts, "luts", torch.uint8).numel() % 768:
            raise AdaispError(f"{what}: luts holds {luts.numel()} bytes, not a whole number of 768-byte tables")
        n_luts = luts.numel() // 768
    for t, name in ((desc, "desc"), (luts, "luts"), (out, "out")):
        if t is not None and isinstance(t, torch.Tensor) and t.device != src.device:
            raise AdaispError(f"{what}: src on {src.device}, {name} on {t.device}")
    if scalar_error is not None:
        raise AdaispError(f"{what}: {scalar_error}")
    if records is not None:
        if not isinstance(records, np.ndarray) or records.dtype != dtype or records.ndim != 1 or len(records) != B:
            raise AdaispError(f"{what}: records must be a 1-D numpy array of {B} {what[:-3].upper()}_DESC")
        check(records, src.numel(), n_luts, S)
    if out is None:
        out = torch.empty((max(B, 1), max(S, 1), max(S, 1), 3), dtype=torch.uint8, device=src.device)
    elif _on_device(what, out, "out", torch.uint8).numel() != B * S * S * 3:
        raise AdaispError(f"{what}: out holds {out.numel()} bytes, {B} frames of {S} x {S} x 3 need {B * S * S * 3}")
    with torch.cuda.device(src.device):
        rc = getattr(L, "adaisp_" + what)(src.data_ptr(), src.numel(), desc.data_ptr(), None if not n_luts else luts.data_ptr(),
                                          n_luts, out.data_ptr(), B, S, int(scalar), _stream())
    _check(rc, "adaisp_" + what)
    _wrote(out)
    return out


def augment_u8(src, desc, luts, S, fill=0, out=None, records=None):
    """adaisp_augment_u8: uint8 HWC BGR images packed in the device byte tensor `src` (any offset: a slice is fine), each
    letterboxed into an S x S frame of colour `fill` (B | G << 8 | R << 16), warped through its Q16 inverse map and, with a
    table, re-coloured in HSV -> uint8 [B,S,S,3] on the device. `desc`: B records of AUGMENT_DESC as a device byte tensor;
    `luts`: the 768-byte tables (hue, saturation, value) as a device byte tensor, or None when no record names one;
    `records` (host, optional): the same records as a numpy array, checked against the buffers before any device work.
    `out`: any contiguous uint8 device tensor of B * S * S * 3 elements."""
    bad = isinstance(fill, bool) or not isinstance(fill, (int, np.integer)) or not 0 <= fill <= 0xFFFFFF
    return _warp_u8("augment_u8", AUGMENT_DESC, _check_augment_records, fill,
                    f"fill must be one BGR triple packed in 24 bits, got {fill!r}" if bad else None, src, desc, luts, S, out, records)


# adaisp_mosaic_desc (include/adaisp.h): one 448-byte record per image: 2 layers of 216 bytes, each 4 tiles of 40
MOSAIC_TILE = np.dtype([("src_offset", "<i8"), ("h", "<i4"), ("w", "<i4"), ("x0", "<i4"), ("y0", "<i4"), ("x1", "<i4"),
                        ("y1", "<i4"), ("dx", "<i4"), ("dy", "<i4")], align=True)
MOSAIC_LAYER = np.dtype([("m", "<i8", (6,)), ("fill", "<u4"), ("n_tiles", "<i4"), ("tile", MOSAIC_TILE, (4,))], align=True)
MOSAIC_DESC = np.dtype([("layer", MOSAIC_LAYER, (2,)), ("n_layers", "<i4"), ("mix", "<i4"), ("lut", "<i4"),
                        ("reserved", "<i4")], align=True)
assert MOSAIC_TILE.itemsize == 40 and MOSAIC_LAYER.itemsize == 216 and MOSAIC_DESC.itemsize == 448
MOSAIC_MIX_ONE = 65536


def _check_mosaic_records(records, src_bytes, n_luts, n_layers=2):
    """What adaisp_mosaic_u8 would take into range or treat as an absent tile, or a map it would wrap, is an error here, and
    a record of more layers than the launch's `n_layers`."""
    r = records
    if np.any((r["n_layers"] < 1) | (r["n_layers"] > 2)):
        raise AdaispError("mosaic_u8: n_layers outside {1, 2}")
    if np.any((r["mix"] < 0) | (r["mix"] > MOSAIC_MIX_ONE)):
        raise AdaispError(f"mosaic_u8: mix outside [0, {MOSAIC_MIX_ONE}]")
    _rule_table("mosaic_u8", r["lut"], n_luts)
    used = np.arange(2)[None, :] < r["n_layers"][:, None]                     # [B,2]: the layers that count
    lay = r["layer"]
    if np.any(used & ((lay["n_tiles"] < 0) | (lay["n_tiles"] > 4))):
        raise AdaispError("mosaic_u8: n_tiles outside [0, 4]")
    if np.any(used & (lay["fill"] > 0xFFFFFF)):
        raise AdaispError("mosaic_u8: fill must be one BGR triple packed in 24 bits")
    _rule_map("mosaic_u8", lay["m"], used[..., None])
    t = lay["tile"]                                                           # [B,2,4]
    live = used[..., None] & (np.arange(4)[None, None, :] < lay["n_tiles"][..., None])
    h, w = t["h"].astype(np.int64), t["w"].astype(np.int64)
    if np.any(live & ((h < 0) | (w < 0) | (h > 32768) | (w > 32768))):
        raise AdaispError("mosaic_u8: a tile's source size outside [0, 32768]")
    x0, y0, x1, y1, dx, dy = (t[k].astype(np.int64) for k in ("x0", "y0", "x1", "y1", "dx", "dy"))
    if np.any(live & ((x1 < x0) | (y1 < y0) | (x0 - dx < 0) | (x1 - dx > w) | (y0 - dy < 0) | (y1 - dy > h))):
        raise AdaispError("mosaic_u8: a tile's rectangle maps outside its own source")
    _rule_inside("mosaic_u8", "a tile's source", t, src_bytes, live)
    if np.any(r["n_layers"] > n_layers):
        raise AdaispError("mosaic_u8: a record of two layers in a launch of n_layers = 1")


def mosaic_u8(src, desc, luts, S, n_layers=2, out=None, records=None):
    """adaisp_mosaic_u8: per image 1 or 2 layers, each a Q16 inverse map over a canvas of up to 4 tiles (uint8 HWC BGR
    sources packed in the device byte tensor `src`, any offset) and a fill; two layers are blended with the record's Q16
    `mix`; then the image's table -> uint8 [B,S,S,3] on the device. `desc`: B records of MOSAIC_DESC as a device byte
    tensor; `luts` as augment_u8's; `n_layers`: 1 when no record has two layers (the second layer's code is not run at all);
    `records` (host, optional): the same records as a numpy array, checked against the buffers before any device work (and
    against n_layers). `out`: any contiguous uint8 device tensor of B * S * S * 3 elements."""
    bad = isinstance(n_layers, bool) or not isinstance(n_layers, (int, np.integer)) or n_layers not in (1, 2)
    return _warp_u8("mosaic_u8", MOSAIC_DESC, lambda r, nbytes, n_luts, S: _check_mosaic_records(r, nbytes, n_luts, n_layers),
                    n_layers, f"n_layers must be 1 or 2, got {n_layers!r}" if bad else None, src, desc, luts, S, out, records)


# adaisp_raw_desc (include/adaisp.h): one 64-byte record per plane
RAW_DESC = np.dtype([("src_offset", "<i8"), ("src_h", "<i4"), ("src_w", "<i4"), ("h", "<i4"), ("w", "<i4"), ("top", "<i4"),
                     ("left", "<i4"), ("tab_x", "<i8"), ("tab_y", "<i8"), ("gain", "<f4", (3,)), ("reserved", "<f4")],
                    align=True)
assert RAW_DESC.itemsize == 64


def raw_load(src, desc, tabs, S, pattern="RGGB", method="bilinear", black_level=0.0, white_level=65535.0, out=None):
    """adaisp_raw_load: native-size uint16 colour-filter-array planes packed in the device byte tensor `src` (even offsets;
    a slice is fine) -> planar fp32 [B,3,S,S]: `demosaic_rects` of each whole plane (same `pattern`, `method`, levels),
    times its gains, resampled through the CSR taps in `tabs` (adaptiveisp_amd/resize.py, RawTapPlan; a device int32 tensor
    or 4-byte aligned bytes) and placed as `desc` (B records of RAW_DESC as a device byte tensor) says, 0 around it. Raises
    on bad arguments before any device work."""
    L, meth = load(), _method("raw_load", method)
    _on_device("raw_load", src, "src", torch.uint8)
    B, S = _records("raw_load", desc, RAW_DESC), int(S)
    tab_words = _tab_words("raw_load", tabs)
    if src.data_ptr() % 2:
        raise AdaispError("raw_load: src must be 2-byte aligned (uint16 samples)")
    if desc.device != src.device or tabs.device != src.device:
        raise AdaispError(f"raw_load: src on {src.device}, desc on {desc.device}, tabs on {tabs.device}")
    out = _out("raw_load", out, (B, 3, S, S), torch.float32, src.device, alloc=(B, 3, max(S, 1), max(S, 1)))
    with torch.cuda.device(src.device):
        rc = L.adaisp_raw_load(src.data_ptr(), src.numel(), desc.data_ptr(), tabs.data_ptr(), tab_words, out.data_ptr(), B, S,
                               _pattern(pattern), meth, float(black_level), float(white_level), _stream())
    _check(rc, "adaisp_raw_load")
    _wrote(out)
    return out


# adaisp_rawfix_desc (include/adaisp.h): one 96-byte record per plane
RAWFIX_DESC = np.dtype([("src_offset", "<i8"), ("dst_offset", "<i8"), ("src_h", "<i4"), ("src_w", "<i4"), ("grid", "<i8"),
                        ("grid_h", "<i4"), ("grid_w", "<i4"), ("step_y", "<f4"), ("step_x", "<f4"), ("black", "<f4", (4,)),
                        ("scale", "<f4", (4,)), ("black_out", "<f4"), ("dpc", "<i4"), ("reserved", "<i4", (2,))], align=True)
assert RAWFIX_DESC.itemsize == 96


def raw_correct(src, desc, gains=None, out=None):
    """adaisp_raw_correct: the uint16 colour-filter-array planes packed in the device byte tensor `src` (even offsets; a
    slice is fine) -> corrected uint16 planes in the device byte tensor `out` (default: a new one of src's size), each as
    its record of `desc` (B records of RAWFIX_DESC as a device byte tensor; adaptiveisp_amd/rawcal.py fills them) says:
    defect pixels, shading gain from the tables in `gains` (a device float32 tensor, or None when no record has one),
    per-position black levels and scale. `out` must not overlap `src`. Raises on bad arguments before any device work."""
    L = load()
    given = [(src, "src", torch.uint8), (desc, "desc", torch.uint8)]
    given += [] if gains is None else [(gains, "gains", torch.float32)]
    given += [] if out is None else [(out, "out", torch.uint8)]
    for t, name, dtype in given:
        if _on_device("raw_correct", t, name, dtype).device != src.device:
            raise AdaispError(f"raw_correct: src on {src.device}, {name} on {t.device}")
    B = _records("raw_correct", desc, RAWFIX_DESC)
    if B > 65535:
        raise AdaispError(f"raw_correct: {B} records, at most 65535 per launch")
    if out is None:
        out = torch.empty(src.numel(), dtype=torch.uint8, device=src.device)
    if src.data_ptr() % 2 or out.data_ptr() % 2:
        raise AdaispError("raw_correct: src and out must be 2-byte aligned (uint16 samples)")
    if src.data_ptr() < out.data_ptr() + out.numel() and out.data_ptr() < src.data_ptr() + src.numel():
        raise AdaispError("raw_correct: out overlaps src (the defect rule reads neighbours: not in place)")
    with torch.cuda.device(src.device):
        rc = L.adaisp_raw_correct(src.data_ptr(), src.numel(), out.data_ptr(), out.numel(), desc.data_ptr(),
                                  None if gains is None else gains.data_ptr(), 0 if gains is None else gains.numel(), B,
                                  _stream())
    _check(rc, "adaisp_raw_correct")
    _wrote(out)
    return out


def export_u8(img, out=None):
    """adaisp_export_u8: planar fp32 RGB [B,3,H,W] on the device -> uint8 HWC BGR [B,H,W,3] on the device, the bytes the
    reference's save_img gives cv2.imwrite (NaN -> 0, clip to [0, 1], * 255 in fp32, round half to even). `out`: any
    uint8 [B,H,W,3] device tensor, contiguous (a view at any byte offset is fine). Raises on bad arguments before any
    device work."""
    L = load()
    img = _dev_f32(img.detach(), "img")
    B, H, W = _img_shape(img)
    out = _out("export_u8", out, (B, H, W, 3), torch.uint8, img.device)
    with torch.cuda.device(img.device):
        rc = L.adaisp_export_u8(img.data_ptr(), out.data_ptr(), B, H, W, _stream())
    _check(rc, "adaisp_export_u8")
    _wrote(out)
    return out


def pack_rggb_to_plane(packed):
    """The reference's 4-channel Bayer packing [..., H/2, W/2, 4] = (R, Gr, Gb, B) (`mosaic`, isp/unprocess_np.py:82-98)
    -> the flat colour-filter-array plane [..., H, W] (`reconstruct_bayer` :111-128 for 'rggb')."""
    h2, w2 = packed.shape[-3], packed.shape[-2]
    plane = packed.new_empty(packed.shape[:-3] + (2 * h2, 2 * w2))
    plane[..., 0::2, 0::2] = packed[..., 0]
    plane[..., 0::2, 1::2] = packed[..., 1]
    plane[..., 1::2, 0::2] = packed[..., 2]
    plane[..., 1::2, 1::2] = packed[..., 3]
    return plane
