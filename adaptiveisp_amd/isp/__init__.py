"""ISP filter stack (host-side mirror of the reference's `isp` package; pixels run in HIP)."""
from .isp_function import image_grad, image_grad_enabled  # noqa: F401
