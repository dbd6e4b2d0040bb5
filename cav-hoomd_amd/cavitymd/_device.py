"""What the user-facing batch classes share when they hand torch objects to ``_capi`` (private)."""
from __future__ import annotations

import numpy as np
import torch


def stream_handle(stream, device) -> int:
    """The raw handle of ``stream``: a torch stream, a raw handle, or None for torch's current stream on ``device``."""
    if stream is None:
        return torch.cuda.current_stream(device).cuda_stream
    return stream.cuda_stream if hasattr(stream, "cuda_stream") else int(stream)


def member_indices(members, n: int, device):
    """(int32 device tensor, count) of ``members``, an index array into a velocity array of ``n`` rows."""
    idx = np.ascontiguousarray(members, dtype=np.uint32)
    if idx.size and int(idx.max()) >= n:
        raise ValueError("a member index lies outside its velocity array")
    return torch.from_numpy(idx.view(np.int32).copy()).to(device), int(idx.shape[0])
