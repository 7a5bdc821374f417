"""Autograd bridge between PyTorch and the C-ABI ISP kernels.

forward  : adaisp_process (one host-known op) or adaisp_forward (per-image op ids on the device)
backward : adaisp_backward_params — gradient w.r.t. the regressed filter parameters. The image gradient
           (adaisp_backward_image) is opt-in: the reference's training treats images as constants
           (train.py:255-258, 341-342), so outside `image_grad()` asking for it raises instead of silently
           returning zeros. Inside it, chained learnable filters, networks upstream of the ISP and the
           detector's data gradient reach the image through the filters.
"""
import contextlib
import threading

import torch

from .. import _lib


def _flat_params(img, param):
    B = img.shape[0]
    p = param.reshape(param.shape[0], -1)
    if p.shape[0] == 1 and B > 1:
        p = p.expand(B, -1)
    if p.shape[0] != B:
        raise ValueError(f"param batch {p.shape[0]} does not match image batch {B}")
    return p.to(torch.float32).contiguous()


_state = threading.local()


def image_grad_enabled():
    """Whether `image_grad()` is active on this thread."""
    return getattr(_state, "enabled", False)


@contextlib.contextmanager
def image_grad(enabled=True):
    """Context manager: ISP filters applied inside it return d(out)/d(img) when the image requires grad (off by default).
    The state is captured when a filter runs FORWARD, so `.backward()` may be called after the block has ended."""
    prev = image_grad_enabled()
    _state.enabled = bool(enabled)
    try:
        yield
    finally:
        _state.enabled = prev


class _IspFunction(torch.autograd.Function):
    @staticmethod
    def forward(ctx, img, params, op_ids, uniform_op, clip):
        if op_ids is None:
            out = _lib.process(uniform_op, img, params, clip=clip)
        else:
            out = _lib.forward(img, op_ids, params, clip=clip)
        ctx.save_for_backward(img, params, op_ids)
        ctx.uniform_op, ctx.clip = uniform_op, clip
        # read here, never in backward: the autograd engine runs device backward passes on a worker thread of its own
        ctx.image_grad = image_grad_enabled()
        return out

    @staticmethod
    def backward(ctx, grad_out):
        img, params, op_ids = ctx.saved_tensors
        if ctx.needs_input_grad[0] and not ctx.image_grad:
            raise NotImplementedError("d(out)/d(img) of the ISP kernels is opt-in: run the forward inside "
                                      "adaptiveisp_amd.image_grad() (the reference's training only differentiates "
                                      "w.r.t. the filter parameters, train.py:341-342)")
        if op_ids is None:
            op_ids = torch.full((img.shape[0],), ctx.uniform_op, dtype=torch.int32, device=img.device)
        grad_img = grad_p = None
        if ctx.needs_input_grad[0]:
            grad_img = _lib.backward_image(img, grad_out, op_ids, params, clip=ctx.clip)
        if ctx.needs_input_grad[1]:
            grad_p = _lib.backward_params(img, grad_out, op_ids, params, clip=ctx.clip)
        return grad_img, grad_p, None, None, None


def isp_apply(img, param, op, clip):
    """One host-known op for the whole batch (Filter.process / Filter.forward)."""
    p = _flat_params(img, param)
    n = _lib.load().adaisp_num_params(int(op))
    if n < 0 or p.shape[1] < n:
        raise ValueError(f"op {op} needs {n} parameters per image, got {p.shape[1]}")
    if torch.is_grad_enabled() and (p.requires_grad or img.requires_grad):
        return _IspFunction.apply(img, p, None, int(op), bool(clip))
    return _lib.process(int(op), img, p, clip=clip)


def isp_apply_selected(img, packed_params, op_ids, clip=True):
    """Per-image ops chosen on the device (Agent.forward): op_ids int32 [B], packed_params [B,stride]."""
    if torch.is_grad_enabled() and (packed_params.requires_grad or img.requires_grad):
        return _IspFunction.apply(img, packed_params.contiguous(), op_ids, 0, bool(clip))
    return _lib.forward(img, op_ids, packed_params, clip=clip)
