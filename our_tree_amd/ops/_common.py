"""What every device op shares: argument checks, byte views, the staging of
misaligned tensors (``_run``) and the single-buffer driver (``_call``).

Every op runs asynchronously on torch's current HIP stream and raises on any
native error.  Tensors may have any dtype; they are treated as contiguous byte
buffers.

numpy stays a lazy import in ``batch_ops``, the one ops module that uses it:
``models.cpu_ref`` and the rest of the package import without it.
"""
from __future__ import annotations

import ctypes
import hmac

import torch

from .. import _native

IMPLS = {"auto": 0, "ttable": 1, "bitslice": 2, "split": 3}  # otc.h OTC_IMPL_*


def _impl(impl) -> int:
    if isinstance(impl, int):
        return impl
    try:
        return IMPLS[impl]
    except KeyError:
        raise ValueError(f"impl must be one of {list(IMPLS)}") from None


def _lib():
    return _native.require_gpu_lib()


def _check_dev(t: torch.Tensor, name: str):
    if not isinstance(t, torch.Tensor):
        raise TypeError(f"{name} must be a torch.Tensor")
    if t.device.type != "cuda":
        raise ValueError(f"{name} must be a GPU tensor (got {t.device})")
    if not t.is_contiguous():
        raise ValueError(f"{name} must be contiguous")


def _nbytes(t: torch.Tensor) -> int:
    return t.numel() * t.element_size()


def _stream(t: torch.Tensor):
    return ctypes.c_void_p(torch.cuda.current_stream(t.device).cuda_stream)


def _bytes(t: torch.Tensor) -> torch.Tensor:
    """Flat uint8 view of a contiguous tensor."""
    return t.reshape(-1).view(torch.uint8)


def _aligned(t: torch.Tensor, a: int = 16) -> torch.Tensor:
    """``t`` for a kernel that loads ``a`` bytes per lane: ``t`` itself, or an
    aligned flat byte copy when it is misaligned and not empty."""
    return _bytes(t).clone() if t.data_ptr() % a and t.numel() else t


def _check_out(out: torch.Tensor, nbytes: int, device, size_msg: str) -> torch.Tensor:
    """A caller's ``out``: a contiguous GPU tensor of ``nbytes`` on ``device``, the input's, where
    the launch goes (another GPU's tensor would be written through a peer address)."""
    _check_dev(out, "out")
    if _nbytes(out) != nbytes:
        raise ValueError(size_msg)
    if out.device != device:
        raise ValueError(f"out must be on the input's device (out is on {out.device}, the input on {device})")
    return out


def _out_like(x: torch.Tensor, out):
    if out is None:
        return torch.empty_like(x)
    return _check_out(out, _nbytes(x), x.device, "out must have the same byte size as the input")


def _run(x: torch.Tensor, out: torch.Tensor, call, inplace_ok: bool = True):
    """call(in_ptr, out_ptr) -> rc.  The kernels move 16 bytes per lane, so the
    native API requires 16-byte aligned buffers; a misaligned tensor (e.g. a
    byte slice ``t[3:]``) is staged through an aligned temporary (torch's
    allocator aligns every fresh allocation) and copied back.  Modes whose
    parallel kernel reads ciphertext block i-1 while block i-1's output is
    written (CBC / CFB decryption, ``inplace_ok=False``) run in place through
    a copy of the input."""
    xp, op = x.data_ptr(), out.data_ptr()
    if not inplace_ok and xp == op and _nbytes(x) > 16:
        x = _bytes(x).clone()
        xp = x.data_ptr()
    if not (xp % 16 or op % 16) or _nbytes(x) == 0:
        return call(xp, op)
    xi = _bytes(x).clone() if xp % 16 else _bytes(x)
    if op == xp:
        xo = xi  # in place stays in place (the native API rejects modes that forbid it)
    elif op % 16:
        xo = torch.empty_like(xi)
    else:
        xo = _bytes(out)
    rc = call(xi.data_ptr(), xo.data_ptr())
    if rc == 0 and xo.data_ptr() != op:
        _bytes(out).copy_(xo)
    return rc


def _call(name: str, x: torch.Tensor, out: torch.Tensor, args, inplace_ok: bool = True, what: str | None = None):
    """The single-buffer driver: the native function ``name`` on ``x``'s
    device, from ``x`` to ``out`` through ``_run``, with the argument tuple
    ``args(in_ptr, out_ptr)``; raises on a native error (named ``what``) and
    returns ``out``.  A conversion inside ``args`` (``_b16``, ``_impl``)
    reports after every check its caller made before."""
    with torch.cuda.device(x.device):
        rc = _run(x, out, lambda ip, op: getattr(_lib(), name)(*args(ip, op)), inplace_ok)
    _native.check(rc, what or name)
    return out


def _b16(v, name) -> ctypes.Array:
    v = bytes(v)
    if len(v) != 16:
        raise ValueError(f"{name} must be 16 bytes")
    return (ctypes.c_uint8 * 16).from_buffer_copy(v)


def _spans(native_name: str) -> list[int]:
    """The boundary list a native ``otc_*_spans(buf, max)`` reports."""
    buf = (ctypes.c_uint64 * 16)()
    n = getattr(_lib(), native_name)(buf, 16)
    return [int(v) for v in buf[:n]]


def _open_with_tag(tag, lengths, length_msg: str, run, exc, mismatch_msg: str) -> torch.Tensor:
    """Authenticated decryption: the received ``tag`` (bytes or a uint8 tensor)
    has one of ``lengths`` bytes; ``run() -> (out, computed tag)``, whose prefix
    is compared in constant time; on a mismatch ``out`` is zeroed and ``exc`` raised.
    A tensor's bytes are read back behind ``run()``'s launches, not in front of them."""
    on_dev = isinstance(tag, torch.Tensor)
    if not on_dev:
        tag = bytes(tag)
    if (_nbytes(tag) if on_dev else len(tag)) not in lengths:
        raise ValueError(length_msg)
    out, t = run()
    if on_dev:
        tag = bytes(tag.cpu().numpy().tobytes())
    if not hmac.compare_digest(t.cpu().numpy().tobytes()[: len(tag)], tag):
        out.zero_()
        raise exc(mismatch_msg)
    return out
