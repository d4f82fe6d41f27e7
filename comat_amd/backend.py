"""The kernel backend object, and the two tensor helpers every host module needs.  The lowest module of the package's host
code: streams, fp8, lora and ops import it, it imports none of them (ops re-exports its names)."""
from . import _hip

_K = None


def kernels():
    global _K
    if _K is None:
        _K = _hip.HipKernels()  # raises if libcomat_hip.so is missing: no fallback
    return _K


def set_kernel_backend(k):
    """Test seam (tests/ only): replace the kernel backend by an object with the HipKernels method set."""
    global _K
    _K = k


def _c(t):
    return t if t.is_contiguous() else t.contiguous()


def _uniform_stride(ts):
    """Element stride between equally shaped, contiguous tensors laid out at a constant spacing inside ONE allocation
    (e.g. dQ / dK / dV of the fused attention backward, or the up factors of a LoRA group), else None."""
    if len(ts) < 2:
        return None
    t0 = ts[0]
    step = ts[1].data_ptr() - t0.data_ptr()
    if step <= 0 or step % t0.element_size():
        return None
    base = t0.untyped_storage().data_ptr()
    for i, t in enumerate(ts):
        if (t.shape != t0.shape or t.dtype != t0.dtype or not t.is_contiguous()
                or t.untyped_storage().data_ptr() != base or t.data_ptr() - t0.data_ptr() != i * step):
            return None
    return step // t0.element_size()
