"""Float64 references of the ISP gradients (adaisp_backward_params, adaisp_backward_image) -- TEST INFRASTRUCTURE ONLY,
like _margins.py and _synth.py.

oracle/torch_ref's filter functions run here in float64: PROCESS[op] is called inside a scoped
torch.set_default_dtype(torch.float64), so the constants it builds without a dtype (_blur3's kernel, USM's linspace, the
HSV buffers) follow the image. torch_ref.process is not used: it casts the parameters to float32. On the GPU the call
also runs under `with torch.device(...)`, since torch_ref builds those constants without a device. ATen's float64 runs
none of this project's kernels, so the reference stays independent of what it checks.

Parameter gradients use forward mode: one torch.func.jvp per parameter column k gives d_k = d out / d p_k per output
element, ref_k = sum G * d_k and S_k = sum |G * d_k|. S_k, the summation mass, is what the error of an fp32 sum of those
terms scales with (|ref_k| can be 1e-3 of it). Forward mode keeps no saved tensors, so NLM fits at 4K.
Image gradients use reverse mode (NLM: the relu restatement of test_imggrad_fixture.py, the reference's own form).

`ambiguity_masks` names the outputs whose kink is decided by arithmetic, where an fp32 kernel may legitimately take the
other side: the float64 value that decides the kink lies within AMBIGUOUS of it. Callers zero grad_out there, in the
tensor that both the kernel and the reference receive. Kinks decided by exact input values (tone / colour breakpoints,
Gamma's 0.001 clip, the input clips, channel ties, NLM's D == 0) are not masked: the header promises a convention for each.
"""
import contextlib

import torch
import torch.nn.functional as F

from oracle import torch_ref
from oracle.torch_ref import CT, NLM, SHR, SHRV2, SP, USM
from test_imggrad_fixture import nlm_relu

# Twice the forward's own tolerance (RTOL = 1e-5 in test_gpu_parity.py): a value the kernel's forward could place on
# the other side of a kink is within this distance of it.
AMBIGUOUS = 2e-5
CLAMPED = (SHR, SHRV2, USM, NLM)          # process already ends in clamp(., 0, 1): the output clip adds no kink


@contextlib.contextmanager
def float64(device):
    prev = torch.get_default_dtype()
    torch.set_default_dtype(torch.float64)
    try:
        with torch.device(device):
            yield
    finally:
        torch.set_default_dtype(prev)


def _params(op, p):
    return p.reshape(p.shape[0], -1)[:, :torch_ref.NUM_PARAMS[op]]


def _f(op, x, p, clip, relu_nlm=False):
    y = nlm_relu(x, p) if (relu_nlm and op == NLM) else torch_ref.PROCESS[op](x, p)
    return torch.clip(y, 0.0, 1.0) if clip else y


def param_grads(op, x, p, grad_out, clip):
    """(ref, S), each float64 [B, NUM_PARAMS[op]]: ref[b, k] = sum grad_out * d out / d p[b, k], S its summation mass."""
    x, G = x.double(), grad_out.double()
    p = _params(op, p.double())
    ref, mass = torch.zeros_like(p), torch.zeros_like(p)
    with float64(x.device):
        for k in range(p.shape[1]):
            t = torch.zeros_like(p)
            t[:, k] = 1.0
            _, d = torch.func.jvp(lambda q: _f(op, x, q, clip), (p,), (t,))
            gd = G * d
            ref[:, k] = gd.sum(dim=(1, 2, 3))
            mass[:, k] = gd.abs().sum(dim=(1, 2, 3))
            del d, gd
    assert torch.isfinite(ref).all() and torch.isfinite(mass).all(), f"op {op}: non-finite reference"
    return ref, mass


def image_grad(op, x, p, grad_out, clip):
    """float64 [B,3,H,W]: d/dx of sum(grad_out * out)."""
    p = _params(op, p.double())
    with float64(x.device):
        xr = x.detach().double().clone().requires_grad_(True)
        y = _f(op, xr, p, clip, relu_nlm=True)
        (y * grad_out.double()).sum().backward()
    g = xr.grad
    assert torch.isfinite(g).all(), f"op {op}: non-finite reference"
    return g


def _pre_clamp(op, x, p):
    """The sharpen pair's and USM's value before their clamp(., 0, 1) (torch_ref.sharpen / sharpen_v2 / usm)."""
    if op == SHR:
        f = p[:, :1, None, None]
        return x * f + torch_ref._blur3(x) * (1 - f)
    if op == SHRV2:
        return x + (x - torch_ref._blur3(x)) * p[:, :1, None, None]
    outs = []
    for b in range(x.shape[0]):
        g = torch.exp(-0.5 * (torch.linspace(-2.0, 2.0, 5) / p[b, 0]) ** 2)
        g = g / g.sum()
        xb = x[b:b + 1]
        blur = F.conv2d(F.pad(xb, (2, 2, 2, 2), mode="reflect"), (g[:, None] * g[None, :]).expand(3, 1, 5, 5), groups=3)
        outs.append(xb + (xb - blur) * p[b, 1])
    return torch.cat(outs, 0)


def _near01(v):
    return (v.abs() < AMBIGUOUS) | ((v - 1.0).abs() < AMBIGUOUS)


def ambiguity_masks(op, x, p):
    """{"process": m, "forward": m}, bool [B,3,H,W]: outputs whose kink is decided by arithmetic (module docstring).
    - the value before the output clip (forward mode; for the ops in CLAMPED that clip passes all of [0, 1]);
    - the value before the internal clamp of Shr, ShrV2, USM and NLM (NLM: num / den, a convex combination of
      clipped colours, so its clamped output is within AMBIGUOUS of an end exactly when the value before is);
    - Contrast's clamp of the luminance;
    - SaturationPlus's sector floor(6h), unless 6h is an integer: that is a channel tie or a grey pixel (4 + 0 / d), exact
      in both precisions. A tie of the maximum is masked, 1e-8 in d / (d + 1e-8) decides it. Its s2 / v clamps never act: v is the max of clipped inputs, an input value, and
      s2 = s + (1 - s) k with 0 <= s <= 1, 0 <= k <= 0.4 stays in [0, 1] under any monotone rounding."""
    x = x.double()
    p = _params(op, p.double())
    with float64(x.device):
        inner = torch.zeros_like(x, dtype=torch.bool)
        if op == CT:
            inner = _near01(torch_ref._lum(x)).expand_as(x)
        elif op == SP:
            h, _, _ = torch_ref._rgb2hsv(torch.clamp(x, 0.0, 1.0))
            h6 = torch.remainder(h, 1.0) * 6.0
            dist = (h6 - torch.round(h6)).abs()
            inner = ((dist > 0) & (dist < AMBIGUOUS))[:, None].expand_as(x)
        elif op in (SHR, SHRV2, USM):
            inner = _near01(_pre_clamp(op, x, p))
        y = torch_ref.PROCESS[op](x, p)
        if op == NLM:
            inner = _near01(y)
        fwd = inner if op in CLAMPED else inner | _near01(y)
    return {"process": inner.contiguous(), "forward": fwd.contiguous()}
