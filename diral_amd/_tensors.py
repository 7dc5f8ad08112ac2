"""What the Python layer hands to the C-ABI of include/diral_env.h by value: raw tensor addresses, dtype codes, 64-bit
seeds - and the one check of a tensor whose address crosses (an int64 or strided tensor would be read as garbage)."""
from __future__ import annotations

from typing import Optional

import torch

U64 = 2**64 - 1

# message forms of `check_tensor` (%-dict templates over name / dtype / shape / dims / device)
MSG_INT32 = "%(name)s must be a contiguous int32 tensor %(dims)s on %(device)s"
MSG_OUT = "%(name)s must be a contiguous %(dtype)s tensor %(shape)s on %(device)s"


def _ptr(t: Optional[torch.Tensor]) -> Optional[int]:
    return None if t is None else t.data_ptr()


def dtype_code(t: torch.Tensor) -> int:
    """config.DT_F64 / DT_F32 of a float tensor."""
    return 1 if t.dtype == torch.float64 else 0


def seed64(seed: int) -> int:
    return int(seed) & U64


def policy_seed(seed: int, k: int) -> int:
    """Seed of the SPS policy's draws number `k` (its step counter, or the offset a device clock is added to)."""
    return (int(seed) * 1000003 + int(k)) & U64


def check_tensor(name: str, t, dtype: torch.dtype, shape: tuple, device: torch.device, msg: str = MSG_INT32) -> None:
    """ValueError unless `t` is a contiguous tensor of `dtype` and `shape` on `device`; `msg` is only formatted then."""
    if not isinstance(t, torch.Tensor) or t.dtype != dtype or tuple(t.shape) != shape or not t.is_contiguous() \
            or t.device != device:
        raise ValueError(msg % dict(name=name, dtype=dtype, shape=shape, dims=list(shape), device=device))
