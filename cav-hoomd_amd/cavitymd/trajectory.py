"""``BatchTrajectoryRecorder`` -- trajectory frames of B independent small systems, appended by ONE kernel launch per call to
a ring of frames in device memory.

What the driver's ``hoomd.write.GSD`` (examples/05_advanced_run.py:1231-1246) saves every ``--gsd-output-period-ps`` with the
initial frame first -- positions, images and velocities -- is one frame per system here (``cavmd_trajectory_header`` and three
packed sections, ``struct cavmd_trajectory_layout``).  Whether a call writes a frame is decided ON THE DEVICE, from the
system's counters and its clock (a ``StepDraw``'s elapsed time), so ``record()`` captured into a graph writes a frame on the
replays where one is due, under an adaptive dt as well, and costs a launch that moves two counters on the others::

    trajectory = BatchTrajectoryRecorder(forces, velocities, capacity=64, time_interval=250.0, clock=draw)
    with torch.cuda.graph(graph):
        draw.fill()
        integrator.step_one(); forces.compute(); coulomb.compute(); integrator.step_two()
        trajectory.record()               # one kernel: a frame of every system whose clock says so
        recorder.record(); thermostat.step_async()
    for _ in range(steps):
        graph.replay()
    frames = trajectory.read()            # (B, n) structured array: header columns, position, velocity, image
    trajectory.unwrapped(frames)          # position + image * box, float64
    trajectory.gsd_chunks(0, -1)          # the last frame of system 0 under GSD's chunk names
    trajectory.save_npz("run.npz")

``dtype="f32"`` stores GSD's chunk types (``(float)x``, round to nearest even, subnormals kept); ``dtype="f64"`` stores exact
copies, and such a frame can be put back into the arrays it came from (``restore``).  Writing ``.gsd`` files is left to the
caller: ``gsd_chunks`` and ``save_npz`` are the hand-over.  There is no CPU fallback: CPU tensors raise.
"""
from __future__ import annotations

import ctypes

import numpy as np
import torch

from . import _capi
from ._device import device_tensor, stream_handle
from .recorder import _SeriesRecorder

_FORMATS = {"f64": _capi.TRAJECTORY_F64, "f32": _capi.TRAJECTORY_F32, "float64": _capi.TRAJECTORY_F64,
            "float32": _capi.TRAJECTORY_F32}


def _sysdefs_of(source):
    """the system definitions of a force batch (anything with ``_sysdefs``) or of a list of them"""
    return list(getattr(source, "_sysdefs", source))


class BatchTrajectoryRecorder(_SeriesRecorder):
    """sysdefs_or_force_batch: the system definitions whose positions, images and boxes are recorded, or a force batch built on
    them; velocities: one (N_k, 4) device tensor per system (mass in column 3), None per system (its velocity section is +0),
    or None for all; capacity: frames an item keeps; period: every ``period``-th ``record()`` writes a frame (the step rule);
    time_interval > 0: a frame whenever the system's clock has advanced by at least that much since its last frame, the first
    call writing one (the time rule; needs ``clock``, a ``StepDraw``, and period 1); dtype: "f32" or "f64"; max_N: the
    particles a frame has room for (default: the largest system)."""

    def __init__(self, sysdefs_or_force_batch, velocities, capacity: int, period: int = 1, time_interval: float = 0.0, clock=None,
                 dtype: str = "f32", max_N=None):
        sysdefs = _sysdefs_of(sysdefs_or_force_batch)
        B = len(sysdefs)
        if B == 0:
            raise ValueError("a trajectory recorder needs at least one system")
        velocities = [None] * B if velocities is None else list(velocities)
        for v in velocities:
            if v is not None:
                device_tensor(v, "BatchTrajectoryRecorder", "velocity")   # CPU tensors are refused before anything else
        pds = [s.getParticleData() for s in sysdefs]
        for pd in pds:
            if pd.device.type != "cuda":
                raise RuntimeError("BatchTrajectoryRecorder needs the position arrays in GPU memory; no CPU fallback exists in "
                                   "this package")
        if len(velocities) != B:
            raise ValueError(f"velocities: None, or one entry per system ({B})")
        if dtype not in _FORMATS:
            raise ValueError('dtype: "f32" or "f64"')
        dev = pds[0].device
        sizes = [pd.getN() for pd in pds]
        for k, (pd, v) in enumerate(zip(pds, velocities)):
            if pd.device != dev or (v is not None and v.device != dev):
                raise ValueError("all systems of one trajectory recorder live on one device")
            if v is not None and v.shape[0] != sizes[k]:
                raise ValueError(f"system {k}: the velocity array has {v.shape[0]} rows, the system {sizes[k]} particles")
        time_ptrs = [0] * B
        if clock is not None:
            if clock.n_systems != B:
                raise ValueError(f"a clock of {clock.n_systems} systems for a trajectory recorder of {B}")
            base = clock._need().state_device_ptr() + _capi.DrawState.elapsed.offset
            time_ptrs = [base + ctypes.sizeof(_capi.DrawState) * i for i in range(B)]
        elif float(time_interval) > 0.0:
            raise ValueError("time_interval > 0 needs a clock (a StepDraw)")
        self.format = _FORMATS[dtype]
        self.max_N = max(max(sizes), 1) if max_N is None else int(max_N)
        # everything whose memory the kernel reads stays alive with the recorder
        self._kept = (sysdefs_or_force_batch, sysdefs, pds, velocities, clock)
        self._pds, self._velocities, self._time_ptrs = pds, velocities, time_ptrs
        items = [self._item(k, pds[k], velocities[k]) for k in range(B)]
        self._open(dev, lambda ws: _capi.Trajectory(ws, items, self.max_N, self.format, capacity, period, time_interval))
        self.n_systems = B
        self.capacity, self.period, self.time_interval = int(capacity), int(period), float(time_interval)
        self.layout = self._handle.layout
        self._record_dtype = lambda: self._handle._RECORD
        self._ones = None
        self._stream = 0
        torch.cuda.current_stream(dev).synchronize()   # ring and counters are zero before any stream records

    def _item(self, k: int, pd, v):
        n = pd.getN()
        return _capi.trajectory_item(pd.getPositions().data_ptr() if n else 0, pd.getImages().data_ptr() if n else 0,
                                     v.data_ptr() if (v is not None and n) else 0, self._time_ptrs[k],
                                     pd.getGlobalBox().getL(), n)

    # -- the launch ------------------------------------------------------------------------------------------------------------
    def record(self, force=False, stream=None) -> None:
        """ONE kernel launch on ``stream`` (default: torch's current stream): nothing is waited for; may be captured.  force:
        False, True (every system writes a frame whatever its rule says) or a (B,) uint32 device tensor of take words, read
        when the kernel runs (a captured call follows what the tensor holds at each replay)."""
        trajectory = self._need()
        take = 0
        if isinstance(force, torch.Tensor):
            if force.device != self._device or force.dtype != torch.uint32 or force.shape != (self.n_systems,) \
                    or not force.is_contiguous():
                raise ValueError(f"force: True, False or a contiguous ({self.n_systems},) uint32 tensor on the recorder's device")
            self._take = force                         # alive while a captured call may read it
            take = force.data_ptr()
        elif force:
            if self._ones is None:
                self._ones = torch.ones(self.n_systems, dtype=torch.int32, device=self._device).view(torch.uint32)
            take = self._ones.data_ptr()
        handle = stream_handle(stream, self._dev_index)
        trajectory.record(handle, take)
        self._stream = handle

    # -- reading ---------------------------------------------------------------------------------------------------------------
    def read(self, first=None, count=None, stream=None) -> np.ndarray:
        """Structured array of shape (B, n): the columns of ``cavmd_trajectory_header`` as (B, n) arrays, ``position`` and
        ``velocity`` as (B, n, max_N, 3) float32 or float64 and ``image`` as (B, n, max_N, 3) int32; frames first .. first +
        count - 1 (0-based count of recorded frames) of every system.  Default: everything still held.  Rows of a section
        beyond a frame's ``N`` are not part of the frame.  Waits for the device (or, if given, for ``stream`` only); never
        inside a capture."""
        return self._read(first, count, stream)

    def unwrapped(self, frames) -> np.ndarray:
        """position + image * box of ``frames`` (what ``read`` returned), float64, shape (..., max_N, 3)"""
        box = np.asarray(frames["box"], dtype=np.float64)[..., None, :]
        return frames["position"].astype(np.float64) + frames["image"].astype(np.float64) * box

    def _frame(self, system: int, row: int) -> np.ndarray:
        """one frame of one system; row < 0 counts from the system's last frame"""
        trajectory = self._need()
        handle = self._read_stream(None)
        if row < 0:
            row += int(trajectory.rows(handle)[system])
            if row < 0:
                raise IndexError("the system has not recorded that many frames")
        return trajectory.read(handle, int(system), 1, int(row), 1)[0, 0]

    def gsd_chunks(self, system: int, row: int = -1) -> dict:
        """One frame of one system under GSD's chunk names: ``configuration/step`` (the call that wrote the frame),
        ``configuration/box``, ``particles/N``, ``particles/position`` and ``particles/velocity`` as float32,
        ``particles/image`` as int32, and the static ``particles/typeid``, ``particles/mass`` and ``particles/charge``."""
        f = self._frame(system, row)
        n = int(f["N"])
        pd, v = self._pds[system], self._velocities[system]
        tags = pd.getPositions()[:n, 3].cpu().numpy().view(np.uint64) & 0xFFFFFFFF
        mass = v[:n, 3].cpu().numpy() if v is not None else np.ones(n)
        return {"configuration/step": np.array([f["call"]], dtype=np.uint64),
                "configuration/box": np.array(list(f["box"]) + [0.0, 0.0, 0.0], dtype=np.float32),
                "particles/N": np.array([n], dtype=np.uint32),
                "particles/position": f["position"][:n].astype(np.float32),
                "particles/velocity": f["velocity"][:n].astype(np.float32),
                "particles/image": f["image"][:n].astype(np.int32),
                "particles/typeid": tags.astype(np.uint32),
                "particles/mass": mass.astype(np.float32),
                "particles/charge": pd.getCharges()[:n].cpu().numpy().astype(np.float32)}

    def save_npz(self, path) -> None:
        """Everything still held, as ``numpy.savez_compressed``: the header columns, ``position``, ``velocity``, ``image``"""
        frames = self.read()
        np.savez_compressed(path, **{name: np.ascontiguousarray(frames[name]) for name in frames.dtype.names})

    # -- putting a frame back --------------------------------------------------------------------------------------------------
    def restore(self, row: int = -1, systems=None) -> None:
        """Writes frame ``row`` (default: the last) of every system in ``systems`` (default: all) back into the arrays it was
        taken from: x, y, z of the positions with the type tags kept, the images, and the velocities with the masses kept.
        For "f64" recorders only (an "f32" frame is not the state); host-driven, refused during a capture.  Forces and
        accelerations are the caller's to evaluate again; to continue a run with the same bits, generators, baths and rings
        included, use ``BatchCheckpoint`` (checkpoint.py)."""
        if self.format != _capi.TRAJECTORY_F64:
            raise RuntimeError('restore() needs exact frames: build the recorder with dtype="f64"')
        if torch.cuda.is_current_stream_capturing():
            raise RuntimeError("restore() copies through the host: it cannot be captured")
        for k in (range(self.n_systems) if systems is None else systems):
            f = self._frame(int(k), int(row))
            pd, v = self._pds[k], self._velocities[k]
            n = int(f["N"])
            if n != pd.getN():
                raise ValueError(f"system {k}: the frame holds {n} particles, the system {pd.getN()}")
            if n == 0:
                continue
            pd.getPositions()[:, :3].copy_(torch.from_numpy(np.ascontiguousarray(f["position"][:n])))
            pd.getImages().copy_(torch.from_numpy(np.ascontiguousarray(f["image"][:n])))
            if v is not None and int(f["flags"]) & _capi.TRAJECTORY_HAS_VELOCITIES:
                v[:, :3].copy_(torch.from_numpy(np.ascontiguousarray(f["velocity"][:n])))
        torch.cuda.current_stream(self._device).synchronize()

    @property
    def trajectory(self):
        return self._handle
