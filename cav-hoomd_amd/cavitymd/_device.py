"""What the user-facing batch classes share when they hand torch objects to ``_capi`` (private): the checks on the tensors
they are given, the stream handle, the owner of a library handle with its workspace, and the step's input rows."""
from __future__ import annotations

import ctypes

import numpy as np
import torch

from . import _capi

_raw_current_stream = getattr(torch._C, "_cuda_getCurrentRawStream", None)


def device_index(device) -> int:
    """The index of a torch device; one without an index is torch's current device."""
    return device.index if device.index is not None else torch.cuda.current_device()


def stream_handle(stream, dev_index: int) -> int:
    """The raw handle of ``stream``: a torch stream, a raw handle, or None for torch's current stream on device ``dev_index``."""
    if stream is None:
        if _raw_current_stream is not None:   # no stream object is built on the per-step path
            return _raw_current_stream(dev_index)
        return torch.cuda.current_stream(dev_index).cuda_stream
    return stream.cuda_stream if hasattr(stream, "cuda_stream") else int(stream)


def device_tensor(t, owner: str, what: str, columns=(4,), note: str = ""):
    """``t`` if it is a contiguous (N, columns) float64 tensor in GPU memory; ``owner`` and ``what`` name the class and the
    array in the message, ``note`` ends it."""
    if not isinstance(t, torch.Tensor) or t.device.type != "cuda":
        raise RuntimeError(f"{owner} needs the {what} arrays in GPU memory; no CPU fallback exists in this package")
    if t.dtype != torch.float64 or t.dim() != 2 or t.shape[1] not in columns or not t.is_contiguous():
        shapes = " or ".join(f"(N,{c})" for c in columns)
        raise ValueError(f"every {what} array must be a contiguous {shapes} float64 tensor{note}")
    return t


def one_device(things, what: str):
    """The device all of ``things`` (tensors, particle data) live on."""
    dev = things[0].device
    if any(t.device != dev for t in things):
        raise ValueError(f"all systems of one {what} live on one device")
    return dev


def per_system(value, n: int, name: str, callables: bool = False):
    """``value`` for each of ``n`` systems: one value (a scalar, None or, with ``callables``, a callable) or one per system."""
    if value is None or np.isscalar(value) or (callables and callable(value)):
        return [value] * n
    value = list(value)
    if len(value) != n:
        raise ValueError(f"{name}: one value, or one per system ({n}), not {len(value)}")
    return value


def member_indices(members, n: int, device):
    """(int32 device tensor, count) of ``members``, an index array into a velocity array of ``n`` rows."""
    idx = np.ascontiguousarray(members, dtype=np.uint32)
    if idx.size and int(idx.max()) >= n:
        raise ValueError("a member index lies outside its velocity array")
    return torch.from_numpy(idx.view(np.int32).copy()).to(device), int(idx.shape[0])


class HandleOwner:
    """A library handle together with the ``Workspace(1)`` it was created from: opened together, used through ``_need()``,
    released together by an idempotent ``close()`` or with the last reference."""
    _handle = _ws = None
    _unusable = "used after close()"

    def _open(self, device, make_handle) -> None:
        """``make_handle(workspace)`` creates the library object; a refusal leaves no workspace behind."""
        self._device = device
        self._dev_index = device_index(device)
        ws = _capi.Workspace(1, device=self._dev_index)
        try:
            self._handle = make_handle(ws)
        except Exception:
            ws.close()
            raise
        self._ws = ws

    def _need(self):
        """The handle, for a launch or a read."""
        if self._handle is None:
            raise RuntimeError(f"{type(self).__name__} {self._unusable}")
        return self._handle

    @property
    def workspace(self) -> _capi.Workspace:
        return self._ws

    def close(self) -> None:
        handle, ws = self._handle, self._ws
        self._handle = self._ws = None
        if handle is not None:
            handle.close()
        if ws is not None:
            ws.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class Checkpointable:
    """``state_dict`` / ``load_state_dict`` of the nine batch classes whose launches write device state (next to
    ``HandleOwner``): the library object's snapshot blob (``cavmd_snapshot_*`` of include/cavmd.h) as one uint8 array under
    ``"snapshot"``, plus the tensors the Python object itself owns and launches write, verbatim.  What the object was built
    from -- the arrays of other owners, parameters, seeds -- is not in there: build the same object first, then load."""

    def _state_tensors(self) -> dict:
        """name -> a tensor, or a list of tensors (one per system), that this object owns and a launch writes"""
        return {}

    def _flat_state_tensors(self) -> dict:
        flat = {}
        for name, value in self._state_tensors().items():
            if isinstance(value, torch.Tensor):
                flat[name] = value
            else:
                flat.update({f"{name}.{k}": t for k, t in enumerate(value)})
        return flat

    def _host_driven(self, what: str) -> None:
        if torch.cuda.is_current_stream_capturing():
            raise RuntimeError(f"{what}() copies through the host: it cannot be captured")

    def state_dict(self, stream=None) -> dict:
        """{"snapshot": the blob, name: array, ...} as numpy arrays.  Default: waits for the whole device (a graph replays on
        the stream it is launched on) first; with ``stream``, for that stream only.  Refused during a capture."""
        handle = self._need()
        self._host_driven("state_dict")
        if stream is None:
            torch.cuda.synchronize(self._device)
        out = {"snapshot": handle.snapshot_save(stream_handle(stream, self._dev_index))}
        for name, t in self._flat_state_tensors().items():
            out[name] = t.detach().cpu().numpy()
        return out

    def check_state_dict(self, d) -> None:
        """Raises ValueError unless ``d`` has exactly this object's names, tensors of its shapes and dtypes, and a blob of its
        kind, system count and size.  Touches nothing (the library checks the blob's remaining words before it loads)."""
        handle = self._need()
        tensors = self._flat_state_tensors()
        who = type(self).__name__
        if set(d) != set(tensors) | {"snapshot"}:
            raise ValueError(f"{who}: the state holds {sorted(d)}, the object {sorted(set(tensors) | {'snapshot'})}")
        for name, t in tensors.items():
            a = np.asarray(d[name])
            if tuple(a.shape) != tuple(t.shape) or torch.from_numpy(np.zeros(0, dtype=a.dtype)).dtype != t.dtype:
                raise ValueError(f"{who}: {name} is {a.dtype}{tuple(a.shape)} in the state, {t.dtype}{tuple(t.shape)} here")
        blob = np.asarray(d["snapshot"])
        if blob.dtype != np.uint8 or blob.ndim != 1 or blob.size < ctypes.sizeof(_capi.SnapshotHeader):
            raise ValueError(f"{who}: the snapshot is no uint8 blob with a header")
        head = _capi.SnapshotHeader.from_buffer_copy(blob[:ctypes.sizeof(_capi.SnapshotHeader)].tobytes())
        kind = _capi.SNAPSHOT_KINDS[handle._PREFIX[len("cavmd_"):]]
        if (head.magic, head.version, head.kind, head.n_items, head.bytes) != \
                (_capi.SNAPSHOT_MAGIC, _capi.SNAPSHOT_VERSION, kind, handle.n_items, blob.size) \
                or blob.size != handle.snapshot_bytes():
            raise ValueError(f"{who}: the snapshot is of another object or shape")

    def load_state_dict(self, d, stream=None) -> None:
        """Puts a ``state_dict`` back: the names, shapes and dtypes are checked, then the library loads the blob (one it refuses
        raises CavmdError and leaves everything as it was), then the tensors are written.  Device addresses do not change: a
        graph captured before replays on the loaded state.  Refused during a capture."""
        handle = self._need()
        self._host_driven("load_state_dict")
        self.check_state_dict(d)
        if stream is None:
            torch.cuda.synchronize(self._device)
        handle.snapshot_load(stream_handle(stream, self._dev_index), np.asarray(d["snapshot"]))
        for name, t in self._flat_state_tensors().items():
            t.copy_(torch.from_numpy(np.ascontiguousarray(d[name])))
        torch.cuda.current_stream(self._device).synchronize()


class StepInputs:
    """The ``(B, 8)`` float64 rows a step kernel reads when it runs.  ``tensor`` is allocated once and never replaced (a
    captured graph holds its address); it starts with a non-zero skip word in column ``skip_column``, so that every system
    is skipped until its inputs are set."""

    def __init__(self, n_systems: int, device, skip_column: int):
        self.tensor = torch.zeros((n_systems, 8), dtype=torch.float64, device=device)
        self.tensor[:, skip_column] = 1.0
        self._pinned = torch.zeros((n_systems, 8), dtype=torch.float64).pin_memory()
        self._copy_done = None
        self._const_key = self._const = None

    def upload(self, rows: np.ndarray) -> None:
        """Host rows reach ``tensor`` with one asynchronous copy on the current stream."""
        if self._copy_done is not None:
            self._copy_done.synchronize()                       # the staging buffer's last copy has left it
        self._pinned.numpy()[:] = rows
        self.tensor.copy_(self._pinned, non_blocking=True)
        self._copy_done = torch.cuda.Event()
        self._copy_done.record(torch.cuda.current_stream(self.tensor.device))

    def fill_constants(self, rows: np.ndarray) -> None:
        """The part of the rows that host arithmetic gives reaches ``tensor`` in stream order, with no host wait; it changes
        rarely and is uploaded only when its bytes did."""
        key = rows.tobytes()
        if self._const_key != key:
            self._const = torch.from_numpy(rows).to(self.tensor.device)
            self._const_key = key
        self.tensor.copy_(self._const)
