"""ctypes binding of csrc/libadayolo.so (C-ABI in include/adayolo.h). No eager/CPU fallback."""
import ctypes
import os

import torch

_HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# ADAYOLO_LIB: another BUILD of the same library (measurement builds of tools/build_variant.py); never a fallback
LIB_PATH = os.environ.get("ADAYOLO_LIB") or os.path.join(_HERE, "csrc", "libadayolo.so")
ABI_VERSION = 10
ACT_NONE, ACT_SILU = 0, 1
EXPORTS = ("adayolo_conv_fwd", "adayolo_conv_fwd_variant", "adayolo_conv_fused1x1_fwd", "adayolo_conv1x1_stream_fwd", "adayolo_bottleneck256_fwd", "adayolo_bottleneck_ws_fwd", "adayolo_conv_keep_fwd", "adayolo_conv_splitk_fwd", "adayolo_conv_dsilu_fwd", "adayolo_conv_s2grad_fwd", "adayolo_conv_splitk_workspace_bytes", "adayolo_conv_chain_workspace_bytes", "adayolo_conv_chain_prepare", "adayolo_conv_chain_fwd", "adayolo_conv_chain_status", "adayolo_conv_chain_poll", "adayolo_conv_chain_tables", "adayolo_stem_fwd", "adayolo_upsample2x", "adayolo_detect_decode", "adayolo_nms", "adayolo_nms_workspace_bytes", "adayolo_match", "adayolo_nms_batch", "adayolo_nms_batch_workspace_bytes", "adayolo_stem_fwd_act", "adayolo_stem_keep_fwd", "adayolo_stem_down_fwd", "adayolo_letterbox_pack", "adayolo_silu_fwd", "adayolo_silu_bwd",
           "adayolo_zero_insert2x", "adayolo_upsample2x_bwd", "adayolo_image_grad", "adayolo_detloss_fwd", "adayolo_detloss_bwd",
           "adayolo_spp_fwd", "adayolo_spp_bwd",
           "adayolo_strerror", "adayolo_set_mfma_shape", "adayolo_get_mfma_shape",
           "adayolo_abi_version")
_lib = None


class AdayoloError(RuntimeError):
    pass


class LossLayer(ctypes.Structure):                 # adayolo_loss_layer (include/adayolo.h)
    _fields_ = [("raw", ctypes.c_void_p), ("cs", ctypes.c_int), ("ny", ctypes.c_int), ("nx", ctypes.c_int),
                ("balance", ctypes.c_float), ("idx", ctypes.c_void_p), ("box", ctypes.c_void_p), ("n", ctypes.c_int),
                ("part", ctypes.c_void_p), ("tobj", ctypes.c_void_p), ("cnt", ctypes.c_void_p),
                ("grad", ctypes.c_void_p), ("grad_cs", ctypes.c_int)]


class ChainLayer(ctypes.Structure):                # adayolo_chain_layer
    _fields_ = [("in_", ctypes.c_void_p), ("in_cstride", ctypes.c_int), ("weight", ctypes.c_void_p), ("bias", ctypes.c_void_p),
                ("residual", ctypes.c_void_p), ("res_cstride", ctypes.c_int), ("out", ctypes.c_void_p), ("out_cstride", ctypes.c_int),
                ("B", ctypes.c_int), ("H", ctypes.c_int), ("W", ctypes.c_int), ("Cin", ctypes.c_int), ("Cout", ctypes.c_int),
                ("ksize", ctypes.c_int), ("stride", ctypes.c_int), ("act", ctypes.c_int), ("weight2", ctypes.c_void_p),
                ("bias2", ctypes.c_void_p), ("out2", ctypes.c_void_p), ("out2_cstride", ctypes.c_int), ("Cout2", ctypes.c_int),
                ("tile", ctypes.c_int)]


class LossArgs(ctypes.Structure):                  # adayolo_loss_args
    _fields_ = [("layer", LossLayer * 4), ("nl", ctypes.c_int), ("B", ctypes.c_int), ("na", ctypes.c_int),
                ("nc", ctypes.c_int), ("no", ctypes.c_int), ("hyp_box", ctypes.c_float), ("hyp_obj", ctypes.c_float),
                ("hyp_cls", ctypes.c_float), ("cp", ctypes.c_float), ("cn", ctypes.c_float), ("cls_pw", ctypes.c_float),
                ("obj_pw", ctypes.c_float), ("loss", ctypes.c_void_p), ("ticket", ctypes.c_void_p),
                ("grad_loss", ctypes.c_void_p)]


class MatchArgs(ctypes.Structure):                 # adayolo_match_args
    _fields_ = [("det", ctypes.c_void_p), ("det_offset", ctypes.c_void_p), ("targets", ctypes.c_void_p),
                ("n_targets", ctypes.c_int32), ("batch", ctypes.c_int32), ("geom", ctypes.c_void_p), ("iouv", ctypes.c_void_p),
                ("n_iou", ctypes.c_int32), ("nc", ctypes.c_int32), ("flags", ctypes.c_int32), ("cm_conf", ctypes.c_float),
                ("cm_iou", ctypes.c_float), ("predn", ctypes.c_void_p), ("correct", ctypes.c_void_p),
                ("confusion", ctypes.c_void_p)]


MATCH_NATIVE = 1


class NmsBatchArgs(ctypes.Structure):              # adayolo_nms_batch_args
    _fields_ = [("pred", ctypes.c_void_p), ("pred_row_stride", ctypes.c_int32), ("B", ctypes.c_int32), ("N", ctypes.c_int32),
                ("nc", ctypes.c_int32), ("conf_thres", ctypes.c_float), ("iou_thres", ctypes.c_float),
                ("max_det", ctypes.c_int32), ("max_nms", ctypes.c_int32), ("cap", ctypes.c_int32), ("flags", ctypes.c_int32),
                ("workspace", ctypes.c_void_p), ("workspace_bytes", ctypes.c_size_t), ("det", ctypes.c_void_p),
                ("det_offset", ctypes.c_void_p), ("status", ctypes.c_void_p)]


NMS_MULTI_LABEL, NMS_AGNOSTIC, NMS_OVERFLOW = 1, 2, 1


def load(path=None):
    """The library with its entry points declared. path: another build of it (the A/B tools), declared the same way and handed
    back without becoming the process's library."""
    global _lib
    if path is None and _lib is not None:
        return _lib
    lib_path = path or LIB_PATH
    if not os.path.exists(lib_path):
        raise AdayoloError(f"{lib_path} not found: run __graft_entry__.build() (hipcc --offload-arch=gfx950); "
                           "the detector has no eager fallback")
    L = ctypes.CDLL(lib_path)
    vp, ci, cf = ctypes.c_void_p, ctypes.c_int, ctypes.c_float
    L.adayolo_conv_fwd.argtypes = [vp, ci, vp, vp, vp, ci, vp, ci, ci, ci, ci, ci, ci, ci, ci, ci, vp]
    L.adayolo_conv_fwd_variant.argtypes = [vp, ci, vp, vp, vp, ci, vp, ci, ci, ci, ci, ci, ci, ci, ci, ci, ci, vp]
    L.adayolo_conv_fwd_variant.restype = ci
    L.adayolo_conv_fused1x1_fwd.argtypes = [vp, ci, vp, vp, vp, ci, vp, ci, ci, ci, ci, ci, ci, ci, ci, ci, vp, vp, vp, ci, ci, vp]
    L.adayolo_conv_fused1x1_fwd.restype = ci
    L.adayolo_bottleneck256_fwd.argtypes = [vp, ci, vp, vp, vp, vp, vp, ci, ci, ci, ci, vp]
    L.adayolo_bottleneck256_fwd.restype = ci
    L.adayolo_bottleneck_ws_fwd.argtypes = [vp, ci, vp, vp, vp, vp, vp, ci, ci, ci, ci, ci, vp]
    L.adayolo_bottleneck_ws_fwd.restype = ci
    L.adayolo_conv_keep_fwd.argtypes = [vp, ci, vp, vp, vp, ci, vp, ci, vp, ci, ci, ci, ci, ci, ci, ci, ci, ci, ci, vp]
    L.adayolo_conv_keep_fwd.restype = ci
    L.adayolo_stem_fwd.argtypes = [vp, vp, vp, vp, ci, ci, ci, ci, ci, ci, cf, ci, vp]
    L.adayolo_upsample2x.argtypes = [vp, ci, vp, ci, ci, ci, ci, ci, vp]
    L.adayolo_detect_decode.argtypes = [vp, ci, vp, ci, ci, vp, cf, ci, ci, ci, ci, ci, vp]
    cl = ctypes.c_long
    L.adayolo_stem_fwd_act.argtypes = [vp, vp, vp, vp, ci, ci, ci, ci, ci, ci, cf, ci, ci, vp]
    L.adayolo_stem_keep_fwd.argtypes = [vp, vp, vp, vp, ci, vp, ci, ci, ci, ci, ci, ci, cf, ci, vp]
    L.adayolo_stem_down_fwd.argtypes = [vp, vp, vp, vp, vp, vp, ci, ci, ci, ci, ci, ci, cf, vp, vp, vp, ci, vp]
    L.adayolo_stem_down_fwd.restype = ci
    L.adayolo_letterbox_pack.argtypes = [vp, vp, ci, ci, ci, ci, ci, ci, cf, vp]
    L.adayolo_letterbox_pack.restype = ci
    L.adayolo_silu_fwd.argtypes = [vp, ci, vp, ci, vp, ci, cl, ci, vp]
    L.adayolo_silu_bwd.argtypes = [vp, ci, vp, ci, vp, ci, vp, ci, ci, cl, ci, vp]
    L.adayolo_zero_insert2x.argtypes = [vp, ci, vp, ci, ci, ci, ci, ci, ci, ci, vp]
    L.adayolo_upsample2x_bwd.argtypes = [vp, ci, vp, ci, ci, ci, ci, ci, ci, vp]
    L.adayolo_image_grad.argtypes = [vp, ci, vp, ci, ci, ci, ci, ci, vp]
    L.adayolo_spp_fwd.argtypes = [vp, ci, vp, ci, ci, ci, ci, ci, vp]
    L.adayolo_spp_bwd.argtypes = [vp, ci, vp, ci, vp, ci, ci, ci, ci, ci, ci, vp]
    for n in ("adayolo_stem_fwd_act", "adayolo_stem_keep_fwd", "adayolo_stem_down_fwd", "adayolo_letterbox_pack", "adayolo_silu_fwd", "adayolo_silu_bwd", "adayolo_zero_insert2x",
              "adayolo_upsample2x_bwd", "adayolo_image_grad", "adayolo_spp_fwd", "adayolo_spp_bwd"):
        getattr(L, n).restype = ci
    for n in ("adayolo_detloss_fwd", "adayolo_detloss_bwd"):
        getattr(L, n).argtypes = [ctypes.POINTER(LossArgs), vp]
        getattr(L, n).restype = ci
    L.adayolo_nms.argtypes = [vp, ci, cf, ci, vp, vp, vp, vp]
    L.adayolo_nms.restype = ci
    L.adayolo_conv_splitk_workspace_bytes.argtypes = [ci] * 8
    L.adayolo_conv_splitk_workspace_bytes.restype = ctypes.c_size_t
    L.adayolo_conv_splitk_fwd.argtypes = [vp, ci, vp, vp, vp, ci, vp, ci, vp, ci, ci, ci, ci, ci, ci, ci, ci, ci, ci, vp,
                                          ctypes.c_size_t, vp]
    L.adayolo_conv_splitk_fwd.restype = ci
    L.adayolo_conv_dsilu_fwd.argtypes = [vp, ci, vp, vp, vp, ci, vp, ci, vp, ci, vp, ci, ci, ci, ci, ci, ci, ci, ci, ci, vp,
                                         ctypes.c_size_t, vp]
    L.adayolo_conv_dsilu_fwd.restype = ci
    L.adayolo_conv_s2grad_fwd.argtypes = [vp, ci, vp, vp, vp, ci, vp, ci, vp, ci, vp, ci, ci, ci, ci, ci, ci, ci, vp, ctypes.c_size_t, vp]
    L.adayolo_conv_s2grad_fwd.restype = ci
    L.adayolo_conv_chain_workspace_bytes.argtypes = [ctypes.POINTER(ChainLayer), ci]
    L.adayolo_conv_chain_workspace_bytes.restype = ctypes.c_size_t
    L.adayolo_conv_chain_prepare.argtypes = [ctypes.POINTER(ChainLayer), ci, vp, ctypes.c_size_t]
    L.adayolo_conv_chain_prepare.restype = ci
    L.adayolo_conv_chain_fwd.argtypes = [ctypes.POINTER(ChainLayer), ci, vp, ctypes.c_size_t, vp]
    L.adayolo_conv_chain_fwd.restype = ci
    L.adayolo_conv_chain_tables.argtypes = [ctypes.POINTER(ChainLayer), ci, vp, ctypes.c_size_t, ctypes.POINTER(ctypes.c_int32)]
    L.adayolo_conv_chain_tables.restype = ci
    L.adayolo_conv_chain_status.argtypes = [vp]
    L.adayolo_conv_chain_status.restype = ci
    L.adayolo_conv1x1_stream_fwd.argtypes = [vp, ci, vp, vp, vp, ci, ci, ci, ci, ci, ci, ci, vp]
    L.adayolo_conv1x1_stream_fwd.restype = ci
    L.adayolo_conv_chain_poll.argtypes = [vp]
    L.adayolo_conv_chain_poll.restype = ci
    L.adayolo_nms_workspace_bytes.argtypes = [ci]
    L.adayolo_nms_workspace_bytes.restype = ctypes.c_size_t
    L.adayolo_match.argtypes = [ctypes.POINTER(MatchArgs), vp]
    L.adayolo_match.restype = ci
    L.adayolo_nms_batch.argtypes = [ctypes.POINTER(NmsBatchArgs), vp]
    L.adayolo_nms_batch.restype = ci
    L.adayolo_nms_batch_workspace_bytes.argtypes = [ci] * 6
    L.adayolo_nms_batch_workspace_bytes.restype = ctypes.c_size_t
    L.adayolo_set_mfma_shape.argtypes = [ci, ci]
    L.adayolo_set_mfma_shape.restype = ci
    L.adayolo_get_mfma_shape.argtypes = [ci]
    L.adayolo_get_mfma_shape.restype = ci
    L.adayolo_strerror.argtypes = [ci]
    L.adayolo_strerror.restype = ctypes.c_char_p
    for n in ("adayolo_conv_fwd", "adayolo_stem_fwd", "adayolo_upsample2x", "adayolo_detect_decode",
              "adayolo_abi_version"):
        getattr(L, n).restype = ci
    if L.adayolo_abi_version() != ABI_VERSION:
        raise AdayoloError("libadayolo.so ABI mismatch: rebuild")
    if path is None:
        _lib = L
    return L


def check(rc, what):
    if rc != 0:
        raise AdayoloError(f"{what} failed: {load().adayolo_strerror(rc).decode()} ({rc})")


def stream_ptr():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _f32(t, what, cols=None):
    if not (isinstance(t, torch.Tensor) and t.is_cuda):
        raise AdayoloError(f"adayolo_match: {what} must be a HIP device tensor: there is no CPU path")
    t = t.to(torch.float32).contiguous()
    if cols is not None and (t.ndim != 2 or t.shape[1] != cols):
        raise AdayoloError(f"adayolo_match: {what} must be [n, {cols}], got {tuple(t.shape)}")
    return t


def match(det, det_offset, targets, geom, iouv, nc, native=False, confusion=None, cm_conf=0.25, cm_iou=0.45):
    """adayolo_match (include/adayolo.h) on the current stream: det [K,6], det_offset int32 [B+1], targets [n,6], geom [B,5] (None
    with `native`), iouv [T], all on one HIP device -> (predn fp32 [K,6], correct uint8 [K,T]). `confusion`: int32
    [(nc+1)*(nc+1)] device tensor, added to. One launch, no host synchronisation."""
    det, targets, iouv = _f32(det, "det", 6), _f32(targets, "targets", 6), _f32(iouv, "iouv")
    dev = det.device
    if det_offset.dtype != torch.int32 or det_offset.device != dev or det_offset.ndim != 1 or det_offset.numel() < 1:
        raise AdayoloError("adayolo_match: det_offset must be an int32 [B+1] tensor on det's device")
    det_offset = det_offset.contiguous()
    B, K, T = det_offset.numel() - 1, det.shape[0], iouv.numel()
    a = MatchArgs()
    if not native:
        geom = _f32(geom, "geom", 5)
        if geom.shape[0] != B:
            raise AdayoloError(f"adayolo_match: geom has {geom.shape[0]} rows for {B} images")
        a.geom = geom.data_ptr()
    if confusion is not None:
        if confusion.dtype != torch.int32 or confusion.device != dev or not confusion.is_contiguous() or \
                confusion.numel() != (nc + 1) * (nc + 1):
            raise AdayoloError("adayolo_match: confusion must be a contiguous int32 [(nc+1)*(nc+1)] tensor on det's device")
        a.confusion = confusion.data_ptr()
    # (an empty tensor has no address; the entry wants one even when no image has a detection: the buffers get one row, and with
    # K == 0 the output buffer stands in for `det` — no image owns a row, so none is read or written)
    predn = torch.empty((max(K, 1), 6), dtype=torch.float32, device=dev)
    correct = torch.empty((max(K, 1), T), dtype=torch.uint8, device=dev)
    a.det = det.data_ptr() if K else predn.data_ptr()
    a.det_offset, a.targets, a.n_targets, a.batch = det_offset.data_ptr(), targets.data_ptr() or None, targets.shape[0], B
    a.iouv, a.n_iou, a.nc, a.flags = iouv.data_ptr(), T, int(nc), MATCH_NATIVE if native else 0
    a.cm_conf, a.cm_iou, a.predn, a.correct = float(cm_conf), float(cm_iou), predn.data_ptr(), correct.data_ptr()
    with torch.cuda.device(dev):
        rc = load().adayolo_match(ctypes.byref(a), stream_ptr())
    check(rc, "adayolo_match")
    return predn[:K], correct[:K]


def nms_batch(pred, conf_thres, iou_thres, max_det, max_nms, cap, multi_label, agnostic, workspace=None, out=None):
    """adayolo_nms_batch (include/adayolo.h) on the current stream: pred fp32 [B, N, 5+nc] on a HIP device, rows contiguous (a
    view into a wider buffer is taken as it is: its row stride is handed over) -> (det fp32 [B*max_det, 6], det_offset int32
    [B+1], status int32 [B]); image b's kept rows are det[det_offset[b]:det_offset[b+1]], the rows behind det_offset[B] are
    uninitialised. `workspace`: a uint8 device tensor of at least adayolo_nms_batch_workspace_bytes(...) bytes (default: one
    is allocated); `out`: (det, det_offset, status) to write into, as a captured graph needs them. Four launches, no host
    synchronisation."""
    what = "adayolo_nms_batch"
    if not (isinstance(pred, torch.Tensor) and pred.is_cuda):
        raise AdayoloError(f"{what}: pred must be a HIP device tensor: there is no CPU path")
    if pred.dtype != torch.float32 or pred.ndim != 3 or pred.shape[2] < 6:
        raise AdayoloError(f"{what}: pred must be fp32 [B, N, 5+nc] with nc >= 1, got {pred.dtype} {tuple(pred.shape)}")
    B, N, C = pred.shape
    if B and N and not (pred.stride(2) == 1 and pred.stride(1) >= C and pred.stride(0) == N * pred.stride(1)):
        pred = pred.contiguous()
    dev, stride = pred.device, (pred.stride(1) if B and N else C)
    L = load()
    need = L.adayolo_nms_batch_workspace_bytes(B, N, C - 5, int(cap), int(max_nms), int(max_det))
    if workspace is None:
        workspace = torch.empty(max(need, 8), dtype=torch.uint8, device=dev)
    elif workspace.dtype != torch.uint8 or workspace.device != dev or not workspace.is_contiguous():
        raise AdayoloError(f"{what}: workspace must be a contiguous uint8 tensor on pred's device")
    if out is None:
        # (zeroed: with B == 0 or N == 0 the entry launches nothing and writes nothing)
        out = (torch.empty((max(B * int(max_det), 1), 6), dtype=torch.float32, device=dev),
               torch.zeros(B + 1, dtype=torch.int32, device=dev), torch.zeros(max(B, 1), dtype=torch.int32, device=dev))
    det, det_offset, status = out
    for t, dt, n, name in ((det, torch.float32, B * int(max_det) * 6, "det"), (det_offset, torch.int32, B + 1, "det_offset"),
                           (status, torch.int32, B, "status")):
        if t.dtype != dt or t.device != dev or not t.is_contiguous() or t.numel() < n:
            raise AdayoloError(f"{what}: {name} must be a contiguous {dt} tensor of at least {n} elements on pred's device")
    a = NmsBatchArgs()
    a.pred, a.pred_row_stride, a.B, a.N, a.nc = pred.data_ptr() or det.data_ptr(), stride, B, N, C - 5
    a.conf_thres, a.iou_thres, a.max_det, a.max_nms, a.cap = float(conf_thres), float(iou_thres), int(max_det), int(max_nms), int(cap)
    a.flags = (NMS_MULTI_LABEL if multi_label else 0) | (NMS_AGNOSTIC if agnostic else 0)
    a.workspace, a.workspace_bytes = workspace.data_ptr(), workspace.numel()
    a.det, a.det_offset, a.status = det.data_ptr(), det_offset.data_ptr(), status.data_ptr()
    with torch.cuda.device(dev):
        rc = L.adayolo_nms_batch(ctypes.byref(a), stream_ptr())
    check(rc, what)
    return det, det_offset, status[:B]
