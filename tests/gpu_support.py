"""Small helpers the GPU tests of the batch objects share: the current stream as the C ABI takes it, and bit-for-bit
comparisons.  Importing this module touches no GPU."""
import math

import numpy as np
import torch

from abi_support import bits as scalar_bits


def stream() -> int:
    """the current torch stream, as the integer the C ABI takes"""
    return torch.cuda.current_stream().cuda_stream


def bits(a) -> np.ndarray:
    """the uint64 view of float64 values (an array comes back for a scalar too; abi_support.bits gives a scalar's as an int)"""
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def same(a, b) -> bool:
    """equal bit for bit as float64 arrays: -0.0 differs from 0.0, and a NaN equals only a NaN of the same payload"""
    return bool(np.array_equal(bits(a), bits(b)))


def same_or_both_nan(a, b) -> bool:
    """two scalars: same bits (so -0.0 != 0.0), or both NaN (NaN payloads are not part of any contract)"""
    return scalar_bits(a) == scalar_bits(b) or (math.isnan(a) and math.isnan(b))


def same_bits(a, b) -> bool:
    """the same bytes, whatever the two host arrays' types and shapes"""
    return np.asarray(a).tobytes() == np.asarray(b).tobytes()


def same_bits_on_device(a: torch.Tensor, b: torch.Tensor) -> bool:
    """two tensors of 8-byte elements, compared where they live"""
    return bool(torch.equal(a.view(torch.int64), b.view(torch.int64)))
