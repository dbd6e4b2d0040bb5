"""``BatchCheckpoint`` -- stop a batch run between two replays and take it up again, in another process, with the same bits.

A run of the captured step keeps its state in three places: the arrays of the systems (positions with their type tags, images,
velocities with their masses), the tensors that batch objects own (``VerletBatch.accel``, the input rows) and the device state
of the library objects (Philox counters, elapsed time and last dt, reservoirs, ring counters and rings, stored reference
fields).  ``BatchCheckpoint`` writes all three to one ``.npz`` file and puts them back into objects built the same way::

    checkpoint = BatchCheckpoint(sysdefs, velocities, {"integrator": integrator, "draw": draw, "thermostat": thermostat,
                                                       "recorder": recorder, "ledger": ledger, "trajectory": trajectory})
    for _ in range(steps):
        graph.replay()
        if due():
            checkpoint.save("run.npz")        # one synchronise, then copies; the previous file stays whole until the new one is

    # in a new process: the same constructors with the same arguments (seeds included), then
    checkpoint.load("run.npz")                # before the first replay; capture the graph before or after, as you like

Every later replay then writes what the uninterrupted run would have written.  Not in the file, and the caller's to recreate:
everything an object is BUILT from (item tables, parameters, seeds given per system), the force objects (they keep nothing a
later launch reads) and host-side generators.  ``eval_sequence`` of a recorder row and result-history sequence numbers restart
in a new process; they are diagnostic.  numpy is the only file format.
"""
from __future__ import annotations

import os

import numpy as np
import torch

FORMAT = 1
_SYSTEM_ARRAYS = ("position", "image", "velocity")


def _write_npz(file, arrays: dict) -> None:
    np.savez(file, **arrays)


class BatchCheckpoint:
    """systems: the system definitions of the run (or a force batch built on them); velocities: one (N_k, 4) tensor per
    system; objects: name -> an object with ``state_dict(stream=None)`` and ``load_state_dict(d, stream=None)`` (and, if it
    has one, ``check_state_dict(d)``): the batch objects whose launches write state, under names of your choice."""

    def __init__(self, systems, velocities, objects: dict):
        self._sysdefs = list(getattr(systems, "_sysdefs", systems))
        self._velocities = list(velocities)
        if len(self._velocities) != len(self._sysdefs):
            raise ValueError(f"velocities: one tensor per system ({len(self._sysdefs)})")
        self._objects = dict(objects)
        for name, obj in self._objects.items():
            if "." in name or not (hasattr(obj, "state_dict") and hasattr(obj, "load_state_dict")):
                raise ValueError(f"objects[{name!r}]: a name without '.', an object with state_dict and load_state_dict")

    # -- what is saved ---------------------------------------------------------------------------------------------------------
    def _system_tensors(self, k: int) -> dict:
        pd = self._sysdefs[k].getParticleData()
        return {"position": pd.getPositions(), "image": pd.getImages(), "velocity": self._velocities[k]}

    def _synchronize(self) -> None:
        devices = {t.device for k in range(len(self._sysdefs)) for t in self._system_tensors(k).values() if t.device.type == "cuda"}
        if devices and torch.cuda.is_current_stream_capturing():
            raise RuntimeError("a checkpoint copies through the host: it cannot be captured")
        for dev in devices:
            torch.cuda.synchronize(dev)

    def state(self) -> dict:
        """Everything ``save`` writes, as a flat dict of numpy arrays: ONE synchronise of the device, then every system's
        position tensor (all four columns), images and velocity tensor verbatim, then every object's ``state_dict``."""
        self._synchronize()
        arrays = {"format": np.array([FORMAT], dtype=np.int64), "n_systems": np.array([len(self._sysdefs)], dtype=np.int64)}
        for k in range(len(self._sysdefs)):
            for what, t in self._system_tensors(k).items():
                arrays[f"system.{k}.{what}"] = t.detach().cpu().numpy()
        for name, obj in self._objects.items():
            for key, a in obj.state_dict().items():
                arrays[f"object.{name}.{key}"] = np.asarray(a)
        return arrays

    def save(self, path) -> None:
        """Writes ``state()`` as one ``.npz`` under a temporary name in the directory of ``path`` and moves it into place with
        ``os.replace``: a job killed at any moment leaves the previous file whole, or the new one."""
        arrays = self.state()
        path = os.fspath(path)
        tmp = f"{path}.tmp.{os.getpid()}"
        try:
            with open(tmp, "wb") as f:
                _write_npz(f, arrays)
                f.flush()
                os.fsync(f.fileno())
            os.replace(tmp, path)
        except BaseException:
            try:
                os.remove(tmp)
            except OSError:
                pass
            raise

    # -- putting it back -------------------------------------------------------------------------------------------------------
    def _expected_names(self, arrays) -> set:
        names = {"format", "n_systems"}
        names |= {f"system.{k}.{what}" for k in range(len(self._sysdefs)) for what in _SYSTEM_ARRAYS}
        for name in self._objects:
            prefix = f"object.{name}."
            names |= {key for key in arrays if key.startswith(prefix)} or {prefix + "snapshot"}
        return names

    def check(self, arrays) -> dict:
        """Raises ValueError unless ``arrays`` (what ``state`` gave, or an opened ``.npz``) fits this run: the names, the number
        of systems, every system's N and dtypes, and every object's own check.  Writes nothing.  Returns the objects' parts."""
        keys = set(arrays)
        if "format" not in keys or "n_systems" not in keys:
            raise ValueError("no batch checkpoint: 'format' or 'n_systems' is missing")
        if int(np.asarray(arrays["format"]).reshape(-1)[0]) != FORMAT:
            raise ValueError(f"a checkpoint of format {arrays['format']}, this package reads {FORMAT}")
        n = int(np.asarray(arrays["n_systems"]).reshape(-1)[0])
        if n != len(self._sysdefs):
            raise ValueError(f"the checkpoint holds {n} systems, the run {len(self._sysdefs)}")
        expected = self._expected_names(keys)
        if keys != expected:
            raise ValueError(f"names: missing {sorted(expected - keys)}, unknown {sorted(keys - expected)}")
        for k in range(n):
            for what, t in self._system_tensors(k).items():
                a = arrays[f"system.{k}.{what}"]
                if tuple(a.shape) != tuple(t.shape):
                    raise ValueError(f"system {k}: {what} has shape {tuple(a.shape)} in the checkpoint, {tuple(t.shape)} in the run")
                if torch.from_numpy(np.zeros(0, dtype=a.dtype)).dtype != t.dtype:
                    raise ValueError(f"system {k}: {what} is {a.dtype} in the checkpoint, {t.dtype} in the run")
        parts = {}
        for name, obj in self._objects.items():
            prefix = f"object.{name}."
            parts[name] = {key[len(prefix):]: np.asarray(arrays[key]) for key in keys if key.startswith(prefix)}
            if hasattr(obj, "check_state_dict"):
                obj.check_state_dict(parts[name])
        return parts

    def load_state(self, arrays) -> None:
        """``check(arrays)``, then the system tensors and every object's ``load_state_dict``.  The tensors are written in
        place: a graph captured on them before stays valid."""
        parts = self.check(arrays)
        self._synchronize()
        for k in range(len(self._sysdefs)):
            for what, t in self._system_tensors(k).items():
                t.copy_(torch.from_numpy(np.ascontiguousarray(arrays[f"system.{k}.{what}"])))
        for name, obj in self._objects.items():
            obj.load_state_dict(parts[name])
        self._synchronize()

    def load(self, path) -> None:
        """Reads the ``.npz`` at ``path`` (no pickles) and ``load_state``s it."""
        with np.load(os.fspath(path), allow_pickle=False) as f:
            arrays = {key: f[key] for key in f.files}
        self.load_state(arrays)
