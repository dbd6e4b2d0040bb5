"""ctypes binding of the C ABI declared in ``include/cavmd.h`` (``libcavmd.so``).

This is the only place where Python meets the HIP library.  There is deliberately no CPU or
PyTorch fallback: if the shared library is missing, cannot be loaded, or finds no HIP device,
the caller gets an exception that says so.
"""
from __future__ import annotations

import ctypes
import os
import subprocess
import sys
import threading

_HERE = os.path.dirname(os.path.abspath(__file__))
CSRC_DIR = os.path.normpath(os.path.join(_HERE, "..", "csrc"))
# in-tree build (this repository) first; next to this file when installed into HOOMD's python tree by
# csrc/hoomd_shim/CMakeLists.txt
_INSTALLED = os.path.join(_HERE, "libcavmd.so")
LIB_PATH = _INSTALLED if (os.path.exists(_INSTALLED) and not os.path.isdir(CSRC_DIR)) else os.path.join(CSRC_DIR, "libcavmd.so")

CAVMD_OK = 0
CAVMD_ERR_INVALID_VALUE = -1
CAVMD_ERR_NO_DEVICE = -2
CAVMD_ERR_CAPACITY = -3
CAVMD_ERR_BAD_PARAMS = -4
CAVMD_ERR_NOT_COMPUTED = -5
CAVMD_ERR_SYNC_TIMEOUT = -6
CAVMD_ERR_EXPIRED = -7


class CavmdError(RuntimeError):
    """A non-zero status from libcavmd (the reference throws std::runtime_error in the same places,
    src/CavityForceComputeGPU.cc:106-109, 188-192)."""

    def __init__(self, status: int, message: str, where: str = ""):
        self.status = status
        super().__init__(f"libcavmd {where}: [{status}] {message}")


class Params(ctypes.Structure):
    """cavmd_params == the reference's cavity_force_params (src/CavityForceCompute.h:28-54)."""
    _fields_ = [("omegac", ctypes.c_double), ("couplstr", ctypes.c_double), ("K", ctypes.c_double),
                ("phmass", ctypes.c_double)]

    def as_dict(self) -> dict:
        return {"omegac": self.omegac, "couplstr": self.couplstr, "K": self.K, "phmass": self.phmass}


class Result(ctypes.Structure):
    """cavmd_result (192 bytes)."""
    _fields_ = [("dipole", ctypes.c_double * 3), ("q", ctypes.c_double * 3), ("Dq", ctypes.c_double * 2),
                ("energy", ctypes.c_double * 3), ("photon_force", ctypes.c_double * 3),
                ("dipole_lo", ctypes.c_double * 3), ("photon_idx", ctypes.c_int32),
                ("n_photon_typed", ctypes.c_int32), ("n_particles", ctypes.c_uint32),
                ("n_partials", ctypes.c_uint32), ("sequence", ctypes.c_uint64), ("total_dipole", ctypes.c_double * 3),
                ("reserved", ctypes.c_double)]


class BussiReservoirState(ctypes.Structure):
    """cavmd_bussi_reservoir (src/BussiReservoirThermostat.h:160-165)."""
    _fields_ = [("reservoir_translational", ctypes.c_double), ("reservoir_rotational", ctypes.c_double),
                ("instantaneous_translational", ctypes.c_double), ("instantaneous_rotational", ctypes.c_double)]


class BussiDeviceState(ctypes.Structure):
    """cavmd_bussi_device_state: the on-device thermostat's counters after its last step."""
    _fields_ = [("reservoir_translational", ctypes.c_double), ("instantaneous_translational", ctypes.c_double),
                ("last_alpha", ctypes.c_double), ("last_kinetic_energy", ctypes.c_double), ("steps", ctypes.c_uint64),
                ("refused", ctypes.c_uint64)]


class BatchItem(ctypes.Structure):
    """cavmd_batch_item (128 bytes): one system of a batch; the four arrays are DEVICE pointers."""
    _fields_ = [("d_pos", ctypes.c_void_p), ("d_charge", ctypes.c_void_p), ("d_image", ctypes.c_void_p),
                ("d_force", ctypes.c_void_p), ("Lx", ctypes.c_double), ("Ly", ctypes.c_double), ("Lz", ctypes.c_double),
                ("params", Params), ("N", ctypes.c_uint32), ("L_typeid", ctypes.c_int32), ("reserved", ctypes.c_uint64 * 4)]


class SharedCavityItem(ctypes.Structure):
    """cavmd_shared_cavity_item (128 bytes): cavmd_batch_item with the cavity's id in its first reserved word."""
    _fields_ = [("d_pos", ctypes.c_void_p), ("d_charge", ctypes.c_void_p), ("d_image", ctypes.c_void_p),
                ("d_force", ctypes.c_void_p), ("Lx", ctypes.c_double), ("Ly", ctypes.c_double), ("Lz", ctypes.c_double),
                ("params", Params), ("N", ctypes.c_uint32), ("L_typeid", ctypes.c_int32), ("cavity", ctypes.c_uint32),
                ("reserved0", ctypes.c_uint32), ("reserved", ctypes.c_uint64 * 3)]


class BussiBatchItem(ctypes.Structure):
    """cavmd_bussi_batch_item (64 bytes): one system of a thermostat batch; d_vel / d_members are DEVICE pointers."""
    _fields_ = [("d_vel", ctypes.c_void_p), ("d_members", ctypes.c_void_p), ("n_members", ctypes.c_uint32),
                ("reserved0", ctypes.c_uint32), ("dof_translational", ctypes.c_double), ("reserved", ctypes.c_uint64 * 4)]


class BussiBatchInput(ctypes.Structure):
    """cavmd_bussi_batch_input (64 bytes): one step's inputs of one item; the rows live in DEVICE memory."""
    _fields_ = [("normal_variate", ctypes.c_double), ("gamma_variate", ctypes.c_double), ("c", ctypes.c_double),
                ("set_T", ctypes.c_double), ("skip", ctypes.c_uint64), ("reserved", ctypes.c_uint64 * 3)]


class Record(ctypes.Structure):
    """cavmd_record (128 bytes): one row of a recorder's time series."""
    _fields_ = [("call", ctypes.c_uint64), ("eval_sequence", ctypes.c_uint64), ("energy", ctypes.c_double * 3),
                ("total_dipole", ctypes.c_double * 3), ("q", ctypes.c_double * 3), ("cavity_kinetic", ctypes.c_double),
                ("cavity_temperature", ctypes.c_double), ("kinetic_energy", ctypes.c_double),
                ("force_mass_sum", ctypes.c_double), ("reserved", ctypes.c_double)]


class RecorderItem(ctypes.Structure):
    """cavmd_recorder_item (64 bytes): one system of a recorder; all four pointers are DEVICE pointers."""
    _fields_ = [("d_result", ctypes.c_void_p), ("d_vel", ctypes.c_void_p), ("d_net_force", ctypes.c_void_p),
                ("d_members", ctypes.c_void_p), ("N", ctypes.c_uint32), ("n_members", ctypes.c_uint32),
                ("reserved", ctypes.c_uint64 * 3)]


class FieldRecord(ctypes.Structure):
    """cavmd_field_record (160 bytes): one row of a field recorder's time series."""
    _fields_ = [("call", ctypes.c_uint64), ("n_references", ctypes.c_uint32), ("took_reference", ctypes.c_uint32),
                ("rho2", ctypes.c_double), ("reserved", ctypes.c_double), ("F", ctypes.c_double * 16)]


class FieldItem(ctypes.Structure):
    """cavmd_field_item (64 bytes): one system of a field recorder; d_position is a DEVICE pointer."""
    _fields_ = [("d_position", ctypes.c_void_p), ("position_stride", ctypes.c_uint64), ("N", ctypes.c_uint32),
                ("reserved0", ctypes.c_uint32), ("reserved", ctypes.c_uint64 * 5)]


class VerletItem(ctypes.Structure):
    """cavmd_verlet_item (128 bytes): one system of an integrator batch; all pointers are DEVICE pointers."""
    _fields_ = [("d_pos", ctypes.c_void_p), ("d_image", ctypes.c_void_p), ("d_vel", ctypes.c_void_p),
                ("d_accel", ctypes.c_void_p), ("d_force", ctypes.c_void_p * 4), ("d_net_force", ctypes.c_void_p),
                ("Lx", ctypes.c_double), ("Ly", ctypes.c_double), ("Lz", ctypes.c_double), ("N", ctypes.c_uint32),
                ("langevin_index", ctypes.c_int32), ("reserved", ctypes.c_uint64 * 3)]


class VerletInput(ctypes.Structure):
    """cavmd_verlet_input (64 bytes): one step's inputs of one item; the rows live in DEVICE memory."""
    _fields_ = [("dt", ctypes.c_double), ("langevin_gamma", ctypes.c_double), ("langevin_coeff", ctypes.c_double),
                ("uniform", ctypes.c_double * 3), ("skip", ctypes.c_uint64), ("reserved", ctypes.c_uint64)]


class VerletState(ctypes.Structure):
    """cavmd_verlet_state (32 bytes): one item's counters."""
    _fields_ = [("steps", ctypes.c_uint64), ("out_of_box", ctypes.c_uint64), ("langevin_reservoir", ctypes.c_double),
                ("reserved", ctypes.c_double)]


class BathItem(ctypes.Structure):
    """cavmd_bath_item (64 bytes): the bath of one system of an integrator batch; d_gamma is a DEVICE pointer."""
    _fields_ = [("d_gamma", ctypes.c_void_p), ("seed", ctypes.c_uint64), ("kT", ctypes.c_double), ("N", ctypes.c_uint32),
                ("reserved0", ctypes.c_uint32), ("reserved", ctypes.c_uint64 * 4)]


class BathState(ctypes.Structure):
    """cavmd_bath_state (32 bytes): one item's counters."""
    _fields_ = [("draws", ctypes.c_uint64), ("coupled", ctypes.c_uint64), ("reservoir", ctypes.c_double),
                ("reserved", ctypes.c_double)]


class ThermalizeItem(ctypes.Structure):
    """cavmd_thermalize_item (160 bytes): the start of one system of a batch; all pointers are DEVICE pointers."""
    _fields_ = [("d_vel", ctypes.c_void_p), ("d_members", ctypes.c_void_p), ("d_pos", ctypes.c_void_p),
                ("d_image", ctypes.c_void_p), ("d_result", ctypes.c_void_p), ("seed", ctypes.c_uint64), ("kT", ctypes.c_double),
                ("N", ctypes.c_uint32), ("n_members", ctypes.c_uint32), ("flags", ctypes.c_uint32),
                ("reserved0", ctypes.c_uint32), ("L", ctypes.c_double * 3), ("params", Params),
                ("reserved", ctypes.c_uint64 * 4)]


class ThermalizeState(ctypes.Structure):
    """cavmd_thermalize_state (64 bytes): one item's counters."""
    _fields_ = [("draws", ctypes.c_uint64), ("thermalised", ctypes.c_uint64), ("skipped", ctypes.c_uint64),
                ("momentum", ctypes.c_double * 3), ("photon", ctypes.c_int32), ("reserved0", ctypes.c_uint32),
                ("reserved", ctypes.c_uint64)]


class LedgerItem(ctypes.Structure):
    """cavmd_ledger_item (128 bytes): one system of an energy ledger; all pointers are DEVICE pointers."""
    _fields_ = [("d_result", ctypes.c_void_p), ("d_vel", ctypes.c_void_p), ("d_members", ctypes.c_void_p),
                ("n_members", ctypes.c_uint32), ("N", ctypes.c_uint32), ("d_energy", ctypes.c_void_p * 4),
                ("d_reservoir", ctypes.c_void_p * 4), ("d_time", ctypes.c_void_p), ("dof", ctypes.c_double),
                ("add_cavity_kinetic", ctypes.c_uint32), ("reserved0", ctypes.c_uint32), ("reserved", ctypes.c_uint64)]


class LedgerRow(ctypes.Structure):
    """cavmd_ledger_row (192 bytes): one row of an energy ledger's time series."""
    _fields_ = [("call", ctypes.c_uint64), ("n_terms", ctypes.c_uint32), ("n_reservoirs", ctypes.c_uint32),
                ("time", ctypes.c_double), ("potential", ctypes.c_double * 4), ("cavity", ctypes.c_double * 3),
                ("cavity_potential", ctypes.c_double), ("potential_total", ctypes.c_double), ("kinetic_group", ctypes.c_double),
                ("kinetic_cavity", ctypes.c_double), ("kinetic_total", ctypes.c_double), ("system_total", ctypes.c_double),
                ("reservoir", ctypes.c_double * 4), ("reservoir_total", ctypes.c_double), ("universe_total", ctypes.c_double),
                ("temperature", ctypes.c_double), ("reserved", ctypes.c_double)]


class DrawItem(ctypes.Structure):
    """cavmd_draw_item (160 bytes): one system of a draw object; the four pointers are DEVICE pointers."""
    _fields_ = [("d_verlet_row", ctypes.c_void_p), ("d_bussi_row", ctypes.c_void_p), ("d_records", ctypes.c_void_p),
                ("d_rows", ctypes.c_void_p), ("capacity", ctypes.c_uint64), ("langevin_gamma", ctypes.c_double),
                ("langevin_kT", ctypes.c_double), ("bussi_set_T", ctypes.c_double), ("bussi_tau", ctypes.c_double),
                ("bussi_dof", ctypes.c_double), ("dt_initial", ctypes.c_double), ("tolerance_target", ctypes.c_double),
                ("tolerance_initial", ctypes.c_double), ("tolerance_time_constant", ctypes.c_double),
                ("dt_min", ctypes.c_double), ("dt_max", ctypes.c_double), ("reserved", ctypes.c_uint64 * 4)]


class DrawState(ctypes.Structure):
    """cavmd_draw_state (64 bytes): one item's counters."""
    _fields_ = [("draws", ctypes.c_uint64), ("dt", ctypes.c_double), ("elapsed", ctypes.c_double),
                ("tolerance", ctypes.c_double), ("exhausted", ctypes.c_uint64), ("reserved", ctypes.c_uint64 * 3)]


class MolecularPair(ctypes.Structure):
    """cavmd_molecular_pair (64 bytes): one entry of the pair table, made by cavmd_molecular_pair_make."""
    _fields_ = [("lj1", ctypes.c_double), ("lj2", ctypes.c_double), ("lj1_12", ctypes.c_double), ("lj2_6", ctypes.c_double),
                ("rcutsq", ctypes.c_double), ("eshift", ctypes.c_double), ("reserved", ctypes.c_uint64 * 2)]


class MolecularBondParams(ctypes.Structure):
    """cavmd_molecular_bond_params (16 bytes)."""
    _fields_ = [("K", ctypes.c_double), ("r0", ctypes.c_double)]


class MolecularParams(ctypes.Structure):
    """cavmd_molecular_params (4240 bytes)."""
    _fields_ = [("n_types", ctypes.c_uint32), ("n_bond_types", ctypes.c_uint32), ("reserved", ctypes.c_uint64),
                ("pair", (MolecularPair * 8) * 8), ("bond", MolecularBondParams * 8)]


class MolecularBond(ctypes.Structure):
    """cavmd_molecular_bond (12 bytes)."""
    _fields_ = [("a", ctypes.c_uint32), ("b", ctypes.c_uint32), ("type", ctypes.c_uint32)]


class MolecularItem(ctypes.Structure):
    """cavmd_molecular_item (64 bytes): d_pos / d_force are DEVICE pointers, h_bonds a HOST pointer read during create /
    set_items only."""
    _fields_ = [("d_pos", ctypes.c_void_p), ("d_force", ctypes.c_void_p), ("h_bonds", ctypes.c_void_p), ("Lx", ctypes.c_double),
                ("Ly", ctypes.c_double), ("Lz", ctypes.c_double), ("N", ctypes.c_uint32), ("n_bonds", ctypes.c_uint32),
                ("reserved", ctypes.c_uint64)]


class CoulombItem(ctypes.Structure):
    """cavmd_coulomb_item (96 bytes): d_pos / d_charge / d_force are DEVICE pointers, h_exclusions a HOST pointer (bond-list
    format, type ignored) read during create / set_items only."""
    _fields_ = [("d_pos", ctypes.c_void_p), ("d_charge", ctypes.c_void_p), ("d_force", ctypes.c_void_p),
                ("h_exclusions", ctypes.c_void_p), ("Lx", ctypes.c_double), ("Ly", ctypes.c_double), ("Lz", ctypes.c_double),
                ("kappa", ctypes.c_double), ("r_cut", ctypes.c_double), ("k_cut", ctypes.c_double), ("N", ctypes.c_uint32),
                ("n_exclusions", ctypes.c_uint32), ("reserved", ctypes.c_uint64)]


class TrajectoryItem(ctypes.Structure):
    """cavmd_trajectory_item (64 bytes): one system of a trajectory object; the four pointers are DEVICE pointers."""
    _fields_ = [("d_pos", ctypes.c_void_p), ("d_image", ctypes.c_void_p), ("d_vel", ctypes.c_void_p), ("d_time", ctypes.c_void_p),
                ("Lx", ctypes.c_double), ("Ly", ctypes.c_double), ("Lz", ctypes.c_double), ("N", ctypes.c_uint32),
                ("reserved0", ctypes.c_uint32)]


class TrajectoryHeader(ctypes.Structure):
    """cavmd_trajectory_header (64 bytes): the start of every frame of a trajectory object's ring."""
    _fields_ = [("call", ctypes.c_uint64), ("row", ctypes.c_uint64), ("time", ctypes.c_double), ("N", ctypes.c_uint32),
                ("flags", ctypes.c_uint32), ("box", ctypes.c_double * 3), ("reserved", ctypes.c_uint64)]


class TrajectoryLayout(ctypes.Structure):
    """struct cavmd_trajectory_layout (48 bytes): where the sections of a frame of up to max_N particles lie."""
    _fields_ = [("frame_bytes", ctypes.c_uint64), ("position_offset", ctypes.c_uint64), ("velocity_offset", ctypes.c_uint64),
                ("image_offset", ctypes.c_uint64), ("max_N", ctypes.c_uint32), ("format", ctypes.c_uint32),
                ("element_bytes", ctypes.c_uint32), ("reserved", ctypes.c_uint32)]


TRAJECTORY_F64, TRAJECTORY_F32 = 0, 1
TRAJECTORY_MAX_BYTES = 2 ** 32
TRAJECTORY_FORCED, TRAJECTORY_HAS_VELOCITIES = 1, 2     # cavmd_trajectory_header.flags
COULOMB_MAX_ITEM_N = 2048
COULOMB_MAX_K = 4096
COULOMB_MAX_EXCLUSIONS = 4
EWALD_RECIPROCAL_DIRECT = 0
EWALD_RECIPROCAL_FACTORED = 1
EWALD_RECIPROCAL = {"direct": EWALD_RECIPROCAL_DIRECT, "factored": EWALD_RECIPROCAL_FACTORED}
COULOMB_PART_SHORT, COULOMB_PART_LONG = 1, 2   # CAVMD_COULOMB_PART_*
COULOMB_PARTS = {"short": COULOMB_PART_SHORT, "long": COULOMB_PART_LONG, "both": COULOMB_PART_SHORT | COULOMB_PART_LONG}
MOLECULAR_MAX_ITEM_N = 2048
MOLECULAR_MAX_BONDS = 4
FIELD_MAX_WAVEVECTORS = 256
FIELD_MAX_REFERENCES = 16
BATCH_MAX_ITEMS = 65536
BATCH_MAX_ITEM_N = 65536


def batch_launch_order(sizes):
    """The order in which cavmd_batch_compute starts the systems of a batch: by N descending, ties in item order (the hardware
    hands out workgroups in launch order, so the long systems of a ragged batch go first).  Results stay indexed by item.
    This restates the library's rule (launch_order in csrc/cavmd_item_table.hpp); it does not read the library's table."""
    import numpy as np
    n = np.asarray(list(sizes), dtype=np.int64)
    return [int(i) for i in np.argsort(-n, kind="stable")]


def batch_item(N, pos_ptr, charge_ptr, image_ptr, force_ptr, box_L, L_typeid, params) -> "BatchItem":
    it = BatchItem()
    it.d_pos, it.d_charge, it.d_image, it.d_force = pos_ptr or None, charge_ptr or None, image_ptr or None, force_ptr or None
    it.Lx, it.Ly, it.Lz = float(box_L[0]), float(box_L[1]), float(box_L[2])
    it.params = params
    it.N, it.L_typeid = int(N), int(L_typeid)
    return it


def shared_cavity_item(N, pos_ptr, charge_ptr, image_ptr, force_ptr, box_L, L_typeid, params, cavity) -> "SharedCavityItem":
    it = SharedCavityItem()
    it.d_pos, it.d_charge, it.d_image, it.d_force = pos_ptr or None, charge_ptr or None, image_ptr or None, force_ptr or None
    it.Lx, it.Ly, it.Lz = float(box_L[0]), float(box_L[1]), float(box_L[2])
    it.params = params
    it.N, it.L_typeid, it.cavity = int(N), int(L_typeid), int(cavity)
    return it


def bussi_batch_item(vel_ptr, members_ptr, n_members, dof_translational) -> "BussiBatchItem":
    it = BussiBatchItem()
    it.d_vel, it.d_members = vel_ptr or None, members_ptr or None
    it.n_members, it.dof_translational = int(n_members), float(dof_translational)
    return it


def recorder_item(result_ptr, vel_ptr, net_force_ptr, members_ptr, N, n_members) -> "RecorderItem":
    it = RecorderItem()
    it.d_result, it.d_vel, it.d_net_force, it.d_members = result_ptr or None, vel_ptr or None, net_force_ptr or None, \
        members_ptr or None
    it.N, it.n_members = int(N), int(n_members)
    return it


def field_item(position_ptr, position_stride, N) -> "FieldItem":
    it = FieldItem()
    it.d_position = position_ptr or None
    it.position_stride, it.N = int(position_stride), int(N)
    return it


def verlet_item(N, pos_ptr, image_ptr, vel_ptr, accel_ptr, force_ptrs, net_force_ptr, box_L, langevin_index=-1) -> "VerletItem":
    it = VerletItem()
    it.d_pos, it.d_image, it.d_vel, it.d_accel = pos_ptr or None, image_ptr or None, vel_ptr or None, accel_ptr or None
    force_ptrs = list(force_ptrs)
    if len(force_ptrs) > 4:
        raise ValueError("at most four force arrays per system")
    for k, p in enumerate(force_ptrs):
        it.d_force[k] = p or None
    it.d_net_force = net_force_ptr or None
    it.Lx, it.Ly, it.Lz = float(box_L[0]), float(box_L[1]), float(box_L[2])
    it.N, it.langevin_index = int(N), int(langevin_index)
    return it


def bath_item(gamma_ptr=0, N=0, kT=0.0, seed=0) -> "BathItem":
    """gamma_ptr == 0 with N == 0: no bath on this item."""
    it = BathItem()
    it.d_gamma, it.N = gamma_ptr or None, int(N)
    it.kT, it.seed = float(kT), int(seed)
    return it


THERMALIZE_ZERO_MOMENTUM, THERMALIZE_PLACE_PHOTON, THERMALIZE_FINITE_Q, THERMALIZE_PHOTON_VELOCITY = 1, 2, 4, 8
THERMALIZE_TILE = 512


def thermalize_item(vel_ptr=0, N=0, kT=0.0, seed=0, members_ptr=0, n_members=0, flags=0, pos_ptr=0, image_ptr=0, result_ptr=0,
                    box_L=(0.0, 0.0, 0.0), params=None) -> "ThermalizeItem":
    """members_ptr == 0: the default set (every particle but the photon the result block names)."""
    it = ThermalizeItem()
    it.d_vel, it.d_members, it.N, it.n_members = vel_ptr or None, members_ptr or None, int(N), int(n_members)
    it.d_pos, it.d_image, it.d_result = pos_ptr or None, image_ptr or None, result_ptr or None
    it.kT, it.seed, it.flags = float(kT), int(seed), int(flags)
    it.L[0], it.L[1], it.L[2] = (float(x) for x in box_L)
    if params is not None:
        it.params = params
    return it


def ledger_item(result_ptr=0, vel_ptr=0, members_ptr=0, n_members=0, N=0, energy_ptrs=(), reservoir_ptrs=(), time_ptr=0, dof=0.0,
                add_cavity_kinetic=0) -> "LedgerItem":
    """One system of an energy ledger: up to four force arrays whose .w is summed and up to four addresses of one double."""
    it = LedgerItem()
    it.d_result, it.d_vel, it.d_members, it.d_time = result_ptr or None, vel_ptr or None, members_ptr or None, time_ptr or None
    it.n_members, it.N = int(n_members), int(N)
    for k, p in enumerate(energy_ptrs):
        it.d_energy[k] = p or None
    for k, p in enumerate(reservoir_ptrs):
        it.d_reservoir[k] = p or None
    it.dof, it.add_cavity_kinetic = float(dof), int(add_cavity_kinetic)
    return it


def draw_item(verlet_row_ptr=0, bussi_row_ptr=0, gamma=0.0, kT=0.0, set_T=0.0, tau=0.0, dof=0.0, dt=0.0, records_ptr=0,
              rows_ptr=0, capacity=0, tolerance=0.0, tolerance_initial=0.0, tolerance_time_constant=0.0, dt_min=0.0,
              dt_max=0.0) -> "DrawItem":
    """records_ptr == 0: a fixed dt; otherwise the adaptive rule on that series with `tolerance` as its target."""
    it = DrawItem()
    it.d_verlet_row, it.d_bussi_row = verlet_row_ptr or None, bussi_row_ptr or None
    it.d_records, it.d_rows, it.capacity = records_ptr or None, rows_ptr or None, int(capacity)
    it.langevin_gamma, it.langevin_kT = float(gamma), float(kT)
    it.bussi_set_T, it.bussi_tau, it.bussi_dof = float(set_T), float(tau), float(dof)
    it.dt_initial, it.tolerance_target, it.tolerance_initial = float(dt), float(tolerance), float(tolerance_initial)
    it.tolerance_time_constant, it.dt_min, it.dt_max = float(tolerance_time_constant), float(dt_min), float(dt_max)
    return it


def molecular_item(N, pos_ptr, force_ptr, box_L, bonds=None) -> "MolecularItem":
    """bonds: None or an (n_bonds, 3) array of (a, b, bond type); the item keeps the array alive (``_bonds``) for the call
    that reads it."""
    import numpy as np
    it = MolecularItem()
    it.d_pos, it.d_force = pos_ptr or None, force_ptr or None
    it.Lx, it.Ly, it.Lz = float(box_L[0]), float(box_L[1]), float(box_L[2])
    it.N = int(N)
    b = np.zeros((0, 3), dtype=np.uint32) if bonds is None else np.ascontiguousarray(bonds, dtype=np.uint32).reshape(-1, 3)
    it._bonds = b
    it.h_bonds, it.n_bonds = (b.ctypes.data if len(b) else None), len(b)
    return it


def coulomb_item(N, pos_ptr, charge_ptr, force_ptr, box_L, kappa, r_cut, k_cut, exclusions=None) -> "CoulombItem":
    """exclusions: None or an (n, 2) or (n, 3) array of pairs (a third column is ignored); the item keeps the array alive
    (``_exclusions``) for the call that reads it."""
    import numpy as np
    it = CoulombItem()
    it.d_pos, it.d_charge, it.d_force = pos_ptr or None, charge_ptr or None, force_ptr or None
    it.Lx, it.Ly, it.Lz = float(box_L[0]), float(box_L[1]), float(box_L[2])
    it.kappa, it.r_cut, it.k_cut = float(kappa), float(r_cut), float(k_cut)
    it.N = int(N)
    e = np.zeros((0, 3), dtype=np.uint32)
    if exclusions is not None and len(exclusions):
        pairs = np.asarray(exclusions, dtype=np.uint32)
        pairs = pairs.reshape(-1, pairs.shape[-1] if pairs.ndim == 2 else 2)
        e = np.zeros((len(pairs), 3), dtype=np.uint32)
        e[:, :2] = pairs[:, :2]
    it._exclusions = e
    it.h_exclusions, it.n_exclusions = (e.ctypes.data if len(e) else None), len(e)
    return it


SNAPSHOT_MAGIC = 0x3150414E53564143   # "CAVSNAP1"
SNAPSHOT_VERSION = 1
# CAVMD_SNAPSHOT_<OBJECT>: the `kind` of a blob, by the object's name in cavmd_snapshot_<object>_*
SNAPSHOT_KINDS = {"verlet": 1, "bath": 2, "draw": 3, "thermalize": 4, "bussi_batch": 5, "recorder": 6, "ledger": 7,
                  "trajectory": 8, "field_recorder": 9}


class SnapshotHeader(ctypes.Structure):
    """cavmd_snapshot_header (64 bytes): what every snapshot blob begins with."""
    _fields_ = [("magic", ctypes.c_uint64), ("version", ctypes.c_uint32), ("kind", ctypes.c_uint32),
                ("n_items", ctypes.c_uint32), ("n_counters", ctypes.c_uint32), ("capacity", ctypes.c_uint64),
                ("record_bytes", ctypes.c_uint64), ("word", ctypes.c_uint32 * 2), ("bytes", ctypes.c_uint64),
                ("reserved", ctypes.c_uint32 * 2)]


def trajectory_item(pos_ptr=0, image_ptr=0, vel_ptr=0, time_ptr=0, box_L=(0.0, 0.0, 0.0), N=0) -> "TrajectoryItem":
    """vel_ptr == 0: the velocity section of every frame is +0; time_ptr == 0: time is 0."""
    it = TrajectoryItem()
    it.d_pos, it.d_image, it.d_vel, it.d_time = pos_ptr or None, image_ptr or None, vel_ptr or None, time_ptr or None
    it.Lx, it.Ly, it.Lz = float(box_L[0]), float(box_L[1]), float(box_L[2])
    it.N = int(N)
    return it


_vp, _sz, _dbl, _ci, _cstr = ctypes.c_void_p, ctypes.c_size_t, ctypes.c_double, ctypes.c_int, ctypes.c_char_p
_u32, _u64, _P = ctypes.c_uint32, ctypes.c_uint64, ctypes.POINTER

# Every symbol include/cavmd.h exports, in the header's order: symbol -> (restype, argtypes).  Tests check the header and the
# library against this table, down to the number of parameters: without a prototype ctypes passes a pointer as a C int.
_PROTOTYPES = {
    "cavmd_make_params": (Params, [_dbl, _dbl, _dbl]),
    "cavmd_create": (_ci, [_ci, _sz, _P(_vp)]),
    "cavmd_destroy": (_ci, [_vp]),
    "cavmd_compute_hoomd": (_ci, [_vp, _vp, _sz, _vp, _vp, _vp, _dbl, _dbl, _dbl, _ci, _P(Params), _vp]),
    "cavmd_compute_soa": (_ci, [_vp, _vp, _sz, _vp, _sz, _vp, _sz, _vp, _sz, _vp, _sz, _dbl, _dbl, _dbl, _ci, _P(Params), _vp,
                                 _sz, _vp, _sz]),
    "cavmd_energies": (_ci, [_vp, _P(_dbl * 3)]),
    "cavmd_result_read": (_ci, [_vp, _P(Result)]),
    "cavmd_result_device_ptr": (_ci, [_vp, _P(_vp)]),
    "cavmd_last_sequence": (_ci, [_vp, _P(_u64)]),
    "cavmd_result_at": (_ci, [_vp, _u64, _P(Result)]),
    "cavmd_energies_at": (_ci, [_vp, _u64, _P(_dbl * 3)]),
    "cavmd_batch_item_check": (_ci, [_P(BatchItem)]),
    "cavmd_batch_create": (_ci, [_vp, _sz, _P(BatchItem), _ci, _P(_vp)]),
    "cavmd_batch_destroy": (_ci, [_vp]),
    "cavmd_batch_set_items": (_ci, [_vp, _sz, _sz, _P(BatchItem)]),
    "cavmd_batch_compute": (_ci, [_vp, _vp]),
    "cavmd_batch_last_sequence": (_ci, [_vp, _P(_u64)]),
    "cavmd_batch_results_read": (_ci, [_vp, _P(Result)]),
    "cavmd_batch_results_at": (_ci, [_vp, _u64, _P(Result)]),
    "cavmd_batch_energies_at": (_ci, [_vp, _u64, _vp]),
    "cavmd_batch_results_device_ptr": (_ci, [_vp, _P(_vp)]),
    "cavmd_shared_cavity_item_check": (_ci, [_P(SharedCavityItem)]),
    "cavmd_shared_cavity_table_check": (_ci, [_sz, _P(SharedCavityItem), _P(_u32)]),
    "cavmd_shared_cavity_create": (_ci, [_vp, _sz, _P(SharedCavityItem), _P(_vp)]),
    "cavmd_shared_cavity_destroy": (_ci, [_vp]),
    "cavmd_shared_cavity_set_items": (_ci, [_vp, _sz, _sz, _P(SharedCavityItem)]),
    "cavmd_shared_cavity_compute": (_ci, [_vp, _vp]),
    "cavmd_shared_cavity_last_sequence": (_ci, [_vp, _P(_u64)]),
    "cavmd_shared_cavity_results_read": (_ci, [_vp, _vp, _P(Result)]),
    "cavmd_shared_cavity_results_device_ptr": (_ci, [_vp, _P(_vp)]),
    "cavmd_shared_cavity_cell_dipoles_device_ptr": (_ci, [_vp, _P(_vp)]),
    "cavmd_shared_cavity_count": (_ci, [_vp, _P(_u32)]),
    "cavmd_shared_cavity_carrier": (_ci, [_vp, _u32, _P(_u32)]),
    "cavmd_set_wavevectors": (_ci, [_vp, _sz, _vp]),
    "cavmd_density_field": (_ci, [_vp, _vp, _sz, _vp, _sz]),
    "cavmd_density_field_read": (_ci, [_vp, _vp]),
    "cavmd_cavity_mode": (_ci, [_vp, _vp, _vp, _dbl, _P(_dbl * 4)]),
    "cavmd_force_mass_sum": (_ci, [_vp, _vp, _sz, _vp, _vp, _P(_dbl)]),
    "cavmd_kinetic_energy": (_ci, [_vp, _vp, _vp, _vp, _sz, _P(_dbl)]),
    "cavmd_scale_velocities": (_ci, [_vp, _vp, _vp, _vp, _sz, _dbl]),
    "cavmd_bussi_rescale_factor": (_ci, [_dbl] * 7 + [_P(_dbl)]),
    "cavmd_bussi_step": (_ci, [_P(BussiReservoirState), _dbl, _dbl, _dbl, _dbl, _dbl, _dbl, _dbl, _P(_dbl * 4), _P(_dbl * 2)]),
    "cavmd_bussi_step_device": (_ci, [_vp, _vp, _vp, _vp, _sz] + [_dbl] * 6),
    "cavmd_bussi_device_read": (_ci, [_vp, _P(BussiDeviceState)]),
    "cavmd_bussi_device_reset": (_ci, [_vp, _vp]),
    "cavmd_bussi_batch_item_check": (_ci, [_P(BussiBatchItem)]),
    "cavmd_bussi_batch_input_make": (_ci, [_dbl] * 5 + [_P(BussiBatchInput)]),
    "cavmd_bussi_batch_create": (_ci, [_vp, _sz, _P(BussiBatchItem), _P(_vp)]),
    "cavmd_bussi_batch_destroy": (_ci, [_vp]),
    "cavmd_bussi_batch_set_items": (_ci, [_vp, _sz, _sz, _P(BussiBatchItem)]),
    "cavmd_bussi_batch_step": (_ci, [_vp, _vp, _vp]),
    "cavmd_bussi_batch_last_sequence": (_ci, [_vp, _P(_u64)]),
    "cavmd_bussi_batch_read": (_ci, [_vp, _P(BussiDeviceState)]),
    "cavmd_bussi_batch_reset": (_ci, [_vp, _vp]),
    "cavmd_bussi_batch_state_device_ptr": (_ci, [_vp, _P(_vp)]),
    "cavmd_recorder_item_check": (_ci, [_P(RecorderItem)]),
    "cavmd_recorder_create": (_ci, [_vp, _sz, _P(RecorderItem), _sz, _u64, _dbl, _P(_vp)]),
    "cavmd_recorder_destroy": (_ci, [_vp]),
    "cavmd_recorder_set_items": (_ci, [_vp, _sz, _sz, _P(RecorderItem)]),
    "cavmd_recorder_record": (_ci, [_vp, _vp]),
    "cavmd_recorder_rows": (_ci, [_vp, _vp, _vp]),
    "cavmd_recorder_read": (_ci, [_vp, _vp, _sz, _sz, _u64, _sz, _vp]),
    "cavmd_recorder_reset": (_ci, [_vp, _vp]),
    "cavmd_recorder_device_ptr": (_ci, [_vp, _P(_vp), _P(_vp)]),
    "cavmd_field_recorder_item_check": (_ci, [_P(FieldItem)]),
    "cavmd_field_recorder_create": (_ci, [_vp, _sz, _P(FieldItem), _sz, _vp, _sz, _u64, _u32, _u64, _P(_vp)]),
    "cavmd_field_recorder_destroy": (_ci, [_vp]),
    "cavmd_field_recorder_set_items": (_ci, [_vp, _sz, _sz, _P(FieldItem)]),
    "cavmd_field_recorder_record": (_ci, [_vp, _vp, _vp]),
    "cavmd_field_recorder_rows": (_ci, [_vp, _vp, _vp]),
    "cavmd_field_recorder_read": (_ci, [_vp, _vp, _sz, _sz, _u64, _sz, _vp]),
    "cavmd_field_recorder_read_fields": (_ci, [_vp, _vp, _sz, _vp, _vp, _vp, _P(_u32)]),
    "cavmd_field_recorder_reset": (_ci, [_vp, _vp]),
    "cavmd_field_recorder_device_ptr": (_ci, [_vp, _P(_vp), _P(_vp)]),
    "cavmd_verlet_item_check": (_ci, [_P(VerletItem)]),
    "cavmd_verlet_input_make": (_ci, [_dbl, _dbl, _dbl, _P(_dbl * 3), _P(VerletInput)]),
    "cavmd_verlet_create": (_ci, [_vp, _sz, _P(VerletItem), _P(_vp)]),
    "cavmd_verlet_destroy": (_ci, [_vp]),
    "cavmd_verlet_set_items": (_ci, [_vp, _sz, _sz, _P(VerletItem)]),
    "cavmd_verlet_accelerations": (_ci, [_vp, _vp]),
    "cavmd_verlet_step_one": (_ci, [_vp, _vp, _vp]),
    "cavmd_verlet_step_two": (_ci, [_vp, _vp, _vp]),
    "cavmd_mts_verlet_kick": (_ci, [_vp, _vp, _vp, _vp, _dbl]),
    "cavmd_verlet_read": (_ci, [_vp, _vp, _vp]),
    "cavmd_verlet_reset": (_ci, [_vp, _vp]),
    "cavmd_verlet_state_device_ptr": (_ci, [_vp, _P(_vp)]),
    "cavmd_bath_item_check": (_ci, [_P(BathItem)]),
    "cavmd_bath_create": (_ci, [_vp, _sz, _P(BathItem), _P(_vp)]),
    "cavmd_bath_destroy": (_ci, [_vp]),
    "cavmd_bath_set_items": (_ci, [_vp, _sz, _sz, _P(BathItem)]),
    "cavmd_bath_step_two": (_ci, [_vp, _vp, _vp]),
    "cavmd_bath_read": (_ci, [_vp, _vp, _vp]),
    "cavmd_bath_reset": (_ci, [_vp, _vp]),
    "cavmd_bath_state_device_ptr": (_ci, [_vp, _P(_vp)]),
    "cavmd_ledger_item_check": (_ci, [_P(LedgerItem)]),
    "cavmd_ledger_create": (_ci, [_vp, _sz, _P(LedgerItem), _sz, _u64, _dbl, _P(_vp)]),
    "cavmd_ledger_destroy": (_ci, [_vp]),
    "cavmd_ledger_set_items": (_ci, [_vp, _sz, _sz, _P(LedgerItem)]),
    "cavmd_ledger_record": (_ci, [_vp, _vp]),
    "cavmd_ledger_rows": (_ci, [_vp, _vp, _vp]),
    "cavmd_ledger_read": (_ci, [_vp, _vp, _sz, _sz, _u64, _sz, _vp]),
    "cavmd_ledger_reset": (_ci, [_vp, _vp]),
    "cavmd_ledger_device_ptr": (_ci, [_vp, _P(_vp), _P(_vp)]),
    # (the header declares these eight between the bath's and the ledger's, whose block stays directly behind the bath's here)
    "cavmd_thermalize_item_check": (_ci, [_P(ThermalizeItem)]),
    "cavmd_thermalize_create": (_ci, [_vp, _sz, _P(ThermalizeItem), _P(_vp)]),
    "cavmd_thermalize_destroy": (_ci, [_vp]),
    "cavmd_thermalize_set_items": (_ci, [_vp, _sz, _sz, _P(ThermalizeItem)]),
    "cavmd_thermalize_run": (_ci, [_vp, _vp]),
    "cavmd_thermalize_read": (_ci, [_vp, _vp, _vp]),
    "cavmd_thermalize_reset": (_ci, [_vp, _vp]),
    "cavmd_thermalize_state_device_ptr": (_ci, [_vp, _P(_vp)]),
    "cavmd_draw_item_check": (_ci, [_P(DrawItem)]),
    "cavmd_draw_create": (_ci, [_vp, _u64, _sz, _P(DrawItem), _P(_vp)]),
    "cavmd_draw_destroy": (_ci, [_vp]),
    "cavmd_draw_set_items": (_ci, [_vp, _sz, _sz, _P(DrawItem)]),
    "cavmd_draw_fill": (_ci, [_vp, _vp]),
    "cavmd_draw_read": (_ci, [_vp, _vp, _vp]),
    "cavmd_draw_reset": (_ci, [_vp, _vp]),
    "cavmd_draw_state_device_ptr": (_ci, [_vp, _P(_vp)]),
    "cavmd_molecular_pair_make": (_ci, [_dbl, _dbl, _dbl, _ci, _P(MolecularPair)]),
    "cavmd_molecular_params_check": (_ci, [_P(MolecularParams)]),
    "cavmd_molecular_item_check": (_ci, [_P(MolecularParams), _P(MolecularItem)]),
    "cavmd_molecular_order": (_ci, [_P(_ci), _P(_ci)]),
    "cavmd_molecular_create": (_ci, [_vp, _P(MolecularParams), _sz, _P(MolecularItem), _P(_vp)]),
    "cavmd_molecular_destroy": (_ci, [_vp]),
    "cavmd_molecular_set_items": (_ci, [_vp, _sz, _sz, _P(MolecularItem)]),
    "cavmd_molecular_compute": (_ci, [_vp, _vp]),
    "cavmd_coulomb_item_check": (_ci, [_P(CoulombItem)]),
    "cavmd_coulomb_k_count": (_ci, [_P(CoulombItem), _P(_u32)]),
    "cavmd_coulomb_parameters": (_ci, [_dbl, _dbl, _P(_dbl), _P(_dbl)]),
    "cavmd_coulomb_order": (_ci, [_P(_ci)] * 4),
    "cavmd_coulomb_create": (_ci, [_vp, _sz, _P(CoulombItem), _P(_vp)]),
    "cavmd_coulomb_destroy": (_ci, [_vp]),
    "cavmd_coulomb_set_items": (_ci, [_vp, _sz, _sz, _P(CoulombItem)]),
    "cavmd_coulomb_compute": (_ci, [_vp, _vp]),
    "cavmd_coulomb_structure_device_ptr": (_ci, [_vp, _P(_vp), _P(_P(_u32))]),
    "cavmd_trajectory_item_check": (_ci, [_P(TrajectoryItem)]),
    "cavmd_trajectory_layout": (_ci, [_u32, _u32, _P(TrajectoryLayout)]),
    "cavmd_trajectory_create": (_ci, [_vp, _sz, _P(TrajectoryItem), _u32, _u32, _sz, _u64, _dbl, _P(_vp)]),
    "cavmd_trajectory_destroy": (_ci, [_vp]),
    "cavmd_trajectory_set_items": (_ci, [_vp, _sz, _sz, _P(TrajectoryItem)]),
    "cavmd_trajectory_record": (_ci, [_vp, _vp, _vp]),
    "cavmd_trajectory_rows": (_ci, [_vp, _vp, _vp]),
    "cavmd_trajectory_read": (_ci, [_vp, _vp, _sz, _sz, _u64, _sz, _vp]),
    "cavmd_trajectory_reset": (_ci, [_vp, _vp]),
    "cavmd_trajectory_device_ptr": (_ci, [_vp, _P(_vp), _P(_vp)]),
    "cavmd_profile_enable": (_ci, [_vp, _ci]),
    "cavmd_profile_read": (_ci, [_vp, _P(_dbl * 3), _P(_u64)]),
    "cavmd_profile_samples": (_ci, [_vp, _vp, _sz, _P(_sz)]),
    "cavmd_snapshot_check": (_ci, [_vp, _sz, _P(SnapshotHeader)]),
    "cavmd_snapshot_verlet_bytes": (_ci, [_vp, _P(_sz)]),
    "cavmd_snapshot_verlet_save": (_ci, [_vp, _vp, _vp, _sz]),
    "cavmd_snapshot_verlet_load": (_ci, [_vp, _vp, _vp, _sz]),
    "cavmd_snapshot_bath_bytes": (_ci, [_vp, _P(_sz)]),
    "cavmd_snapshot_bath_save": (_ci, [_vp, _vp, _vp, _sz]),
    "cavmd_snapshot_bath_load": (_ci, [_vp, _vp, _vp, _sz]),
    "cavmd_snapshot_draw_bytes": (_ci, [_vp, _P(_sz)]),
    "cavmd_snapshot_draw_save": (_ci, [_vp, _vp, _vp, _sz]),
    "cavmd_snapshot_draw_load": (_ci, [_vp, _vp, _vp, _sz]),
    "cavmd_snapshot_thermalize_bytes": (_ci, [_vp, _P(_sz)]),
    "cavmd_snapshot_thermalize_save": (_ci, [_vp, _vp, _vp, _sz]),
    "cavmd_snapshot_thermalize_load": (_ci, [_vp, _vp, _vp, _sz]),
    "cavmd_snapshot_bussi_batch_bytes": (_ci, [_vp, _P(_sz)]),
    "cavmd_snapshot_bussi_batch_save": (_ci, [_vp, _vp, _vp, _sz]),
    "cavmd_snapshot_bussi_batch_load": (_ci, [_vp, _vp, _vp, _sz]),
    "cavmd_snapshot_recorder_bytes": (_ci, [_vp, _P(_sz)]),
    "cavmd_snapshot_recorder_save": (_ci, [_vp, _vp, _vp, _sz]),
    "cavmd_snapshot_recorder_load": (_ci, [_vp, _vp, _vp, _sz]),
    "cavmd_snapshot_ledger_bytes": (_ci, [_vp, _P(_sz)]),
    "cavmd_snapshot_ledger_save": (_ci, [_vp, _vp, _vp, _sz]),
    "cavmd_snapshot_ledger_load": (_ci, [_vp, _vp, _vp, _sz]),
    "cavmd_snapshot_trajectory_bytes": (_ci, [_vp, _P(_sz)]),
    "cavmd_snapshot_trajectory_save": (_ci, [_vp, _vp, _vp, _sz]),
    "cavmd_snapshot_trajectory_load": (_ci, [_vp, _vp, _vp, _sz]),
    "cavmd_snapshot_field_recorder_bytes": (_ci, [_vp, _P(_sz)]),
    "cavmd_snapshot_field_recorder_save": (_ci, [_vp, _vp, _vp, _sz]),
    "cavmd_snapshot_field_recorder_load": (_ci, [_vp, _vp, _vp, _sz]),
    "cavmd_set_tunable": (_ci, [_vp, _cstr, _ci]),
    "cavmd_get_tunable": (_ci, [_vp, _cstr, _P(_ci)]),
    "cavmd_runclock_draw_set_end": (_ci, [_vp, _sz, _sz, _P(_dbl)]),
    "cavmd_runclock_draw_finished": (_ci, [_vp, _vp, _P(_u64)]),
    "cavmd_runclock_ledger_set_rule": (_ci, [_vp, _dbl, _dbl]),
    "cavmd_runclock_field_set_rule": (_ci, [_vp, _vp, _u64, _dbl, _dbl]),
    "cavmd_ewald_order": (_ci, [_P(_ci)] * 5),
    "cavmd_ewald_set_reciprocal": (_ci, [_vp, _ci]),
    "cavmd_ewald_get_reciprocal": (_ci, [_vp, _P(_ci)]),
    "cavmd_mts_coulomb_set_long_forces": (_ci, [_vp, _sz, _P(_vp)]),
    "cavmd_mts_coulomb_compute_parts": (_ci, [_vp, _vp, ctypes.c_uint]),
    "cavmd_device_info": (_ci, [_vp, _P(_ci), _P(_ci), _cstr, _sz]),
    "cavmd_error_string": (_cstr, [_ci]),
    "cavmd_version": (_ci, []),
}
EXPORTED_SYMBOLS = tuple(_PROTOTYPES)

_lib = None
_lock = threading.Lock()


def build(force: bool = False) -> str:
    """Compile libcavmd.so for gfx950 with hipcc (cross-compiles without a GPU).  Idempotent."""
    # One make call; make knows from the dependency files written next to the objects what is stale and rebuilds that alone:
    # the product; the same library with the test hooks compiled in (fault injection; loaded by tests only, see
    # load_hooks_build); the product with the lane splits the default build does not cover (loaded by tests only, see
    # load_split_variant); the pybind11 flavour of the shim (cavitymd._cavitymd).
    targets = ["libcavmd.so", "libcavmd_hooks.so", "split_variants", "pymod"]
    jobs = min(16, os.cpu_count() or 1)
    subprocess.run(["make", "-C", CSRC_DIR, "-s", f"-j{jobs}"] + (["-B"] if force else []) + targets, check=True)
    return LIB_PATH


def load():
    """Load libcavmd.so and declare its prototypes.  Raises if the library is not there."""
    global _lib
    with _lock:
        if _lib is not None:
            return _lib
        if not os.path.exists(LIB_PATH):
            raise ImportError(
                f"{LIB_PATH} is missing: build it with `make -C {CSRC_DIR}` (or `python -c 'import __graft_entry__ as g; "
                "g.build()'`).  The cavity force has no CPU/PyTorch fallback in this package.")
        _lib = _declare(ctypes.CDLL(LIB_PATH))
        return _lib


_hooks_lib = None
HOOKS_LIB_PATH = os.path.join(CSRC_DIR, "libcavmd_hooks.so")


def load_hooks_build():
    """TESTS ONLY: libcavmd_hooks.so, the same sources compiled with -DCAVMD_TEST_HOOKS (fault-injecting instantiations of the
    single-launch kernel and the debug_* tunables that drive them).  The product library has neither."""
    global _hooks_lib
    with _lock:
        if _hooks_lib is None:
            if not os.path.exists(HOOKS_LIB_PATH):
                raise ImportError(f"{HOOKS_LIB_PATH} is missing: build it with `make -C {CSRC_DIR} hooks`")
            _hooks_lib = _declare(ctypes.CDLL(HOOKS_LIB_PATH))
        return _hooks_lib


# name -> (CAVMD_MOLECULAR_J_SPLIT, CAVMD_COULOMB_J_SPLIT, CAVMD_COULOMB_K_SPLIT) of libcavmd_split_<name>.so (csrc/Makefile)
SPLIT_VARIANTS = {"a": (1, 1, 1), "b": (4, 4, 16), "c": (16, 64, 64)}
_split_libs = {}


def split_variant_path(name: str) -> str:
    if name not in SPLIT_VARIANTS:
        raise ValueError(f"no split variant {name!r}: one of {sorted(SPLIT_VARIANTS)}")
    return os.path.join(CSRC_DIR, f"libcavmd_split_{name}.so")


def load_split_variant(name: str):
    """TESTS ONLY: libcavmd_split_<name>.so, the same sources compiled with other lane splits (SPLIT_VARIANTS), so that every
    value include/cavmd.h allows runs in some test.  The product path never loads one."""
    path = split_variant_path(name)
    with _lock:
        if name not in _split_libs:
            if not os.path.exists(path):
                raise ImportError(f"{path} is missing: build it with `make -C {CSRC_DIR} split_variants`")
            _split_libs[name] = _declare(ctypes.CDLL(path))
        return _split_libs[name]


def _declare(lib):
    """Gives every exported symbol of ``lib`` (the product, hooks or a split-variant build) its prototype."""
    for name, (restype, argtypes) in _PROTOTYPES.items():
        fn = getattr(lib, name)
        fn.restype, fn.argtypes = restype, argtypes
    return lib


def error_string(status: int) -> str:
    return load().cavmd_error_string(int(status)).decode()


def check(status: int, where: str = "") -> None:
    if status != CAVMD_OK:
        raise CavmdError(status, error_string(status), where)


def bussi_rescale_factor(K, degrees_of_freedom, deltaT, set_T, tau, normal_variate, gamma_variate) -> float:
    out = ctypes.c_double()
    check(load().cavmd_bussi_rescale_factor(float(K), float(degrees_of_freedom), float(deltaT), float(set_T), float(tau),
                                            float(normal_variate), float(gamma_variate), ctypes.byref(out)),
          "cavmd_bussi_rescale_factor")
    return float(out.value)


def bussi_step(state: BussiReservoirState, K_trans, dof_trans, K_rot, dof_rot, deltaT, set_T, tau, variates):
    v = (ctypes.c_double * 4)(*[float(x) for x in variates])
    f = (ctypes.c_double * 2)()
    check(load().cavmd_bussi_step(ctypes.byref(state), float(K_trans), float(dof_trans), float(K_rot), float(dof_rot),
                                  float(deltaT), float(set_T), float(tau), ctypes.byref(v), ctypes.byref(f)), "cavmd_bussi_step")
    return float(f[0]), float(f[1])


def make_params(omegac: float, couplstr: float, phmass: float = 1.0) -> Params:
    return load().cavmd_make_params(float(omegac), float(couplstr), float(phmass))


# Workspaces released while a stream capture was under way, destroyed at the next release or creation outside one.  Python
# may collect a dropped workspace at any allocation, inside a capture too (torch.cuda.graph does not collect before it
# captures); the frees of cavmd_destroy would invalidate that capture.
_deferred = []
# The same for the objects created from a workspace (batches, thermostat batches, recorders, field recorders), as
# (destroy entry point, handle): always emptied before _deferred, the workspaces they were created from.
_deferred_children = []
# The same for the baths created from an integrator: always emptied before _deferred_children, the integrators among them.
_deferred_baths = []


def _capturing() -> bool:
    """True while the current stream of this thread is being captured into a graph."""
    torch = sys.modules.get("torch")
    try:
        return torch is not None and torch.cuda.is_initialized() and torch.cuda.is_current_stream_capturing()
    except Exception:
        return False


def _destroy_deferred() -> None:
    while _deferred_baths:       # a bath goes before the integrator it was created from, whichever was closed first
        destroy, h = _deferred_baths.pop()
        destroy(h)
    while _deferred_children:
        destroy, h = _deferred_children.pop()
        destroy(h)
    while _deferred:
        lib, h = _deferred.pop()
        lib.cavmd_destroy(h)


def _destroy_deferred_outside_capture() -> None:
    if (_deferred_baths or _deferred_children or _deferred) and not _capturing():
        _destroy_deferred()


class Workspace:
    """Owns one cavmd_workspace (scratch for partial sums + the 192-byte result block)."""

    def __init__(self, max_N: int, device: int = -1, hooks: bool = False, lib=None):
        """lib: TESTS ONLY, a library loaded by load_split_variant; what is created from the workspace runs that build."""
        if not _capturing():
            _destroy_deferred()
        if lib is not None and hooks:
            raise ValueError("either the hooks build or a given library")
        self._lib = lib if lib is not None else (load_hooks_build() if hooks else load())
        self._h = ctypes.c_void_p()
        check(self._lib.cavmd_create(int(device), int(max_N), ctypes.byref(self._h)), "cavmd_create")
        self.max_N = int(max_N)

    @property
    def handle(self):
        return self._h

    def close(self):
        if getattr(self, "_h", None) is not None and self._h.value:
            if _capturing():
                _deferred.append((self._lib, self._h))
            else:
                if _deferred_children:  # children deferred during a capture go before any workspace
                    _destroy_deferred()
                self._lib.cavmd_destroy(self._h)
            self._h = ctypes.c_void_p()
        _destroy_deferred_outside_capture()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # -- hot path -----------------------------------------------------------------------------------
    def compute_hoomd(self, stream: int, N: int, pos_ptr: int, charge_ptr: int, image_ptr: int, box_L, L_typeid: int,
                      params: Params, force_ptr: int) -> None:
        check(
            self._lib.cavmd_compute_hoomd(self._h, ctypes.c_void_p(stream), int(N), ctypes.c_void_p(pos_ptr),
                                          ctypes.c_void_p(charge_ptr), ctypes.c_void_p(image_ptr), float(box_L[0]),
                                          float(box_L[1]), float(box_L[2]), int(L_typeid), ctypes.byref(params),
                                          ctypes.c_void_p(force_ptr)), "cavmd_compute_hoomd")

    def compute_soa(self, stream: int, N: int, position, typeid, image, charge, box_L, L_typeid: int, params: Params,
                    force, potential_energy=None) -> None:
        """Each array argument is a (device_pointer, stride_in_bytes) pair."""
        pe_ptr, pe_stride = potential_energy if potential_energy is not None else (None, 0)
        check(
            self._lib.cavmd_compute_soa(self._h, ctypes.c_void_p(stream), int(N), ctypes.c_void_p(position[0]),
                                        int(position[1]), ctypes.c_void_p(typeid[0]), int(typeid[1]),
                                        ctypes.c_void_p(image[0]), int(image[1]), ctypes.c_void_p(charge[0]),
                                        int(charge[1]), float(box_L[0]), float(box_L[1]), float(box_L[2]),
                                        int(L_typeid), ctypes.byref(params), ctypes.c_void_p(force[0]), int(force[1]),
                                        ctypes.c_void_p(pe_ptr), int(pe_stride)), "cavmd_compute_soa")

    # -- results ------------------------------------------------------------------------------------
    def energies(self):
        out = (ctypes.c_double * 3)()
        check(self._lib.cavmd_energies(self._h, ctypes.byref(out)), "cavmd_energies")
        return float(out[0]), float(out[1]), float(out[2])

    def result(self) -> Result:
        r = Result()
        check(self._lib.cavmd_result_read(self._h, ctypes.byref(r)), "cavmd_result_read")
        return r

    def last_sequence(self) -> int:
        """Sequence number of the last evaluation enqueued (0 before any); no wait."""
        out = ctypes.c_uint64()
        check(self._lib.cavmd_last_sequence(self._h, ctypes.byref(out)), "cavmd_last_sequence")
        return int(out.value)

    def result_at(self, sequence: int) -> Result:
        """Result block of evaluation `sequence`, from its slot of the result ring: waits for that evaluation only."""
        r = Result()
        check(self._lib.cavmd_result_at(self._h, int(sequence), ctypes.byref(r)), "cavmd_result_at")
        return r

    def energies_at(self, sequence: int):
        out = (ctypes.c_double * 3)()
        check(self._lib.cavmd_energies_at(self._h, int(sequence), ctypes.byref(out)), "cavmd_energies_at")
        return float(out[0]), float(out[1]), float(out[2])

    def result_device_ptr(self) -> int:
        p = ctypes.c_void_p()
        check(self._lib.cavmd_result_device_ptr(self._h, ctypes.byref(p)), "cavmd_result_device_ptr")
        return int(p.value)

    # -- observables -----------------------------------------------------
    def set_wavevectors(self, wavevectors) -> None:
        import numpy as np
        k = np.ascontiguousarray(wavevectors, dtype=np.float64)
        if k.ndim != 2 or k.shape[1] != 3:
            raise ValueError("wavevectors must have shape (n_k, 3)")
        self._n_k = int(k.shape[0])
        check(self._lib.cavmd_set_wavevectors(self._h, self._n_k, ctypes.c_void_p(k.ctypes.data)), "cavmd_set_wavevectors")

    def density_field(self, stream: int, N: int, position_ptr: int, position_stride: int) -> None:
        check(self._lib.cavmd_density_field(self._h, ctypes.c_void_p(stream), int(N), ctypes.c_void_p(position_ptr),
                                            int(position_stride)), "cavmd_density_field")

    def density_field_read(self):
        import numpy as np
        out = np.empty(2 * self._n_k, dtype=np.float64)
        check(self._lib.cavmd_density_field_read(self._h, ctypes.c_void_p(out.ctypes.data)), "cavmd_density_field_read")
        return out[0::2] + 1j * out[1::2]

    def cavity_mode(self, stream: int, vel_ptr: int, kB: float):
        out = (ctypes.c_double * 4)()
        check(self._lib.cavmd_cavity_mode(self._h, ctypes.c_void_p(stream), ctypes.c_void_p(vel_ptr), float(kB),
                                          ctypes.byref(out)), "cavmd_cavity_mode")
        return float(out[0]), float(out[1]), float(out[2]), float(out[3])

    def force_mass_sum(self, stream: int, N: int, force_ptr: int, vel_ptr: int) -> float:
        out = ctypes.c_double()
        check(self._lib.cavmd_force_mass_sum(self._h, ctypes.c_void_p(stream), int(N), ctypes.c_void_p(force_ptr),
                                             ctypes.c_void_p(vel_ptr), ctypes.byref(out)), "cavmd_force_mass_sum")
        return float(out.value)

    def kinetic_energy(self, stream: int, vel_ptr: int, members_ptr, n_members: int) -> float:
        out = ctypes.c_double()
        check(self._lib.cavmd_kinetic_energy(self._h, ctypes.c_void_p(stream), ctypes.c_void_p(vel_ptr),
                                             ctypes.c_void_p(members_ptr) if members_ptr else None, int(n_members),
                                             ctypes.byref(out)), "cavmd_kinetic_energy")
        return float(out.value)

    def scale_velocities(self, stream: int, vel_ptr: int, members_ptr, n_members: int, alpha: float) -> None:
        check(self._lib.cavmd_scale_velocities(self._h, ctypes.c_void_p(stream), ctypes.c_void_p(vel_ptr),
                                               ctypes.c_void_p(members_ptr) if members_ptr else None, int(n_members),
                                               float(alpha)), "cavmd_scale_velocities")

    def bussi_step_device(self, stream: int, vel_ptr: int, members_ptr, n_members: int, dof: float, deltaT: float, set_T: float,
                          tau: float, normal_variate: float, gamma_variate: float) -> None:
        """One translational thermostat step on the device, asynchronous (two kernels, no host round trip)."""
        check(self._lib.cavmd_bussi_step_device(self._h, ctypes.c_void_p(stream), ctypes.c_void_p(vel_ptr),
                                                ctypes.c_void_p(members_ptr) if members_ptr else None, int(n_members),
                                                float(dof), float(deltaT), float(set_T), float(tau), float(normal_variate),
                                                float(gamma_variate)), "cavmd_bussi_step_device")

    def bussi_device_read(self) -> "BussiDeviceState":
        out = BussiDeviceState()
        check(self._lib.cavmd_bussi_device_read(self._h, ctypes.byref(out)), "cavmd_bussi_device_read")
        return out

    def bussi_device_reset(self, stream: int = 0) -> None:
        check(self._lib.cavmd_bussi_device_reset(self._h, ctypes.c_void_p(stream)), "cavmd_bussi_device_reset")

    # -- measurement / tuning -----------------------------------------------------------------------
    def profile_enable(self, on: bool) -> None:
        check(self._lib.cavmd_profile_enable(self._h, 1 if on else 0), "cavmd_profile_enable")

    def profile_read(self):
        ms = (ctypes.c_double * 3)()
        n = ctypes.c_uint64()
        check(self._lib.cavmd_profile_read(self._h, ctypes.byref(ms), ctypes.byref(n)), "cavmd_profile_read")
        return [float(ms[0]), float(ms[1]), float(ms[2])], int(n.value)

    def profile_samples(self, cap: int = 4096):
        """(n, 3) array of per-evaluation kernel times in ms {reduce, finalize, map}; call before profile_read()."""
        import numpy as np
        out = np.empty((cap, 3), dtype=np.float64)
        n = ctypes.c_size_t()
        check(self._lib.cavmd_profile_samples(self._h, ctypes.c_void_p(out.ctypes.data), int(cap), ctypes.byref(n)),
              "cavmd_profile_samples")
        return out[:n.value].copy()

    def set_tunable(self, name: str, value: int) -> None:
        check(self._lib.cavmd_set_tunable(self._h, name.encode(), int(value)), f"cavmd_set_tunable({name})")

    def get_tunable(self, name: str) -> int:
        v = ctypes.c_int()
        check(self._lib.cavmd_get_tunable(self._h, name.encode(), ctypes.byref(v)), f"cavmd_get_tunable({name})")
        return int(v.value)

    def device_info(self) -> dict:
        dev, cu = ctypes.c_int(), ctypes.c_int()
        buf = ctypes.create_string_buffer(64)
        check(self._lib.cavmd_device_info(self._h, ctypes.byref(dev), ctypes.byref(cu), buf, 64), "cavmd_device_info")
        return {"device": dev.value, "compute_units": cu.value, "arch": buf.value.decode()}


class _ItemTableHandle:
    """What the thirteen batch objects share (Batch, SharedCavity, BussiBatch, Recorder, FieldRecorder, Verlet, Bath, Thermalize,
    Ledger, Draw, Molecular, Coulomb and Trajectory): a handle created from a workspace (kept alive here) over a table of items, released outside stream captures
    only.  A subclass names its item structure, its ``cavmd_*`` prefix and the size the library sorts its launch order by.
    Nothing here relies on ``__init__`` having run."""
    _ITEM = None    # the ctypes structure of one item
    _PREFIX = None  # entry points <prefix>_create, <prefix>_destroy, <prefix>_set_items
    _size = None    # item -> the size key of the launch order
    _DEFERRED = "_deferred_children"  # the module's list that takes a handle closed during a stream capture

    def _call(self, name, *args) -> None:
        """<prefix>_<name>(handle, *args), its status checked; for what is not called per step"""
        check(getattr(self._lib, f"{self._PREFIX}_{name}")(self._h, *args), f"{self._PREFIX}_{name}")

    def _create(self, workspace: Workspace, items, *args, before=()) -> None:
        """<prefix>_create(workspace, *before, n_items, items, *args, &handle)"""
        self._ws = workspace
        self._lib = workspace._lib
        items = list(items)
        self.n_items = len(items)
        self.sizes = [self._size(it) for it in items]
        self._h = ctypes.c_void_p()
        check(getattr(self._lib, self._PREFIX + "_create")(workspace.handle, *before, self.n_items, self._array(items), *args,
                                                            ctypes.byref(self._h)), self._PREFIX + "_create")

    def _array(self, items):
        return (self._ITEM * max(len(items), 1))(*items)   # at least one element: a ctypes array cannot be empty

    @property
    def handle(self):
        return self._h

    @property
    def launch_order(self):
        """Item indices in the order their workgroups start (size key descending, stable), as PREDICTED from the sizes by
        ``batch_launch_order``: the rule the library sorts by, restated in Python, not a read-back of the table the library
        uploaded (results do not depend on the order; it matters for load balance only)."""
        return batch_launch_order(self.sizes)

    def close(self):
        if getattr(self, "_h", None) is not None and self._h.value:
            destroy = getattr(self._lib, self._PREFIX + "_destroy")
            if _capturing():
                globals()[self._DEFERRED].append((destroy, self._h))
            else:
                destroy(self._h)
            self._h = ctypes.c_void_p()
        _destroy_deferred_outside_capture()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def set_items(self, first: int, items) -> None:
        items = list(items)
        self._call("set_items", int(first), len(items), self._array(items))
        for k, it in enumerate(items):
            self.sizes[first + k] = self._size(it)


def snapshot_check(blob, expected: SnapshotHeader) -> int:
    """Status cavmd_snapshot_<object>_load would give `blob` (a uint8 array or bytes) for an object whose header is `expected`,
    from the blob's first 64 bytes (host arithmetic only: needs no device)."""
    import numpy as np
    b = np.ascontiguousarray(np.frombuffer(blob, dtype=np.uint8) if isinstance(blob, (bytes, bytearray)) else blob, dtype=np.uint8)
    return int(load().cavmd_snapshot_check(ctypes.c_void_p(b.ctypes.data) if b.size else None, int(b.size), ctypes.byref(expected)))


class _Snapshots:
    """What the nine handles whose launches write device state share (the state and the series handles, and BussiBatch): that
    state as one blob in host memory, cavmd_snapshot_<object>_bytes / _save / _load of include/cavmd.h."""

    def _snapshot(self, name):
        return getattr(self._lib, "cavmd_snapshot_" + self._PREFIX[len("cavmd_"):] + "_" + name), \
            "cavmd_snapshot_" + self._PREFIX[len("cavmd_"):] + "_" + name

    def snapshot_bytes(self) -> int:
        fn, where = self._snapshot("bytes")
        n = ctypes.c_size_t()
        check(fn(self._h, ctypes.byref(n)), where)
        return int(n.value)

    def snapshot_save(self, stream: int = 0):
        """The object's device state after synchronising `stream`: header and arrays, a uint8 array."""
        import numpy as np
        out = np.zeros(self.snapshot_bytes(), dtype=np.uint8)
        fn, where = self._snapshot("save")
        check(fn(self._h, ctypes.c_void_p(stream), ctypes.c_void_p(out.ctypes.data), int(out.size)), where)
        return out

    def snapshot_load(self, stream: int, blob) -> None:
        """Puts a blob of ``snapshot_save`` back; one of another kind or shape raises CavmdError(CAVMD_ERR_INVALID_VALUE) and
        leaves the object as it was."""
        import numpy as np
        b = np.ascontiguousarray(blob, dtype=np.uint8).reshape(-1)
        fn, where = self._snapshot("load")
        check(fn(self._h, ctypes.c_void_p(stream), ctypes.c_void_p(b.ctypes.data) if b.size else None, int(b.size)), where)


class _SeriesHandle(_ItemTableHandle, _Snapshots):
    """A handle whose launches append rows to a time series in device memory (SeriesTable in csrc/cavmd_item_table.hpp).  A
    subclass names the ctypes structure of one row."""
    _RECORD = None

    def rows(self, stream: int = 0):
        """Rows written per item since creation / reset, after synchronising `stream` (a uint64 array of n_items)."""
        import numpy as np
        out = np.zeros(self.n_items, dtype=np.uint64)
        self._call("rows", ctypes.c_void_p(stream), ctypes.c_void_p(out.ctypes.data))
        return out

    def read(self, stream: int, first_item: int, n_items: int, first_row: int, n_rows: int):
        """Rows first_row .. first_row + n_rows - 1 of items first_item .. first_item + n_items - 1, after synchronising
        `stream`: a structured array of shape (n_items, n_rows) with the layout of the row structure."""
        import numpy as np
        out = np.zeros((max(int(n_items), 0), max(int(n_rows), 0)), dtype=np.dtype(self._RECORD))
        self._call("read", ctypes.c_void_p(stream), int(first_item), int(n_items), int(first_row), int(n_rows),
                   ctypes.c_void_p(out.ctypes.data))
        return out

    def reset(self, stream: int = 0) -> None:
        self._call("reset", ctypes.c_void_p(stream))

    def device_ptr(self):
        """(series, rows): device addresses of the series (item-major, `capacity` rows each) and of the row counters."""
        rec, rows = ctypes.c_void_p(), ctypes.c_void_p()
        self._call("device_ptr", ctypes.byref(rec), ctypes.byref(rows))
        return int(rec.value), int(rows.value)


class _StateHandle(_ItemTableHandle, _Snapshots):
    """A handle with one state per item in device memory (StateTable in csrc/cavmd_item_table.hpp).  A subclass names the
    ctypes structure of one state."""
    _STATE = None

    def read(self, stream: int = 0):
        """The n_items states after synchronising `stream`: a structured array with the layout of the state structure."""
        import numpy as np
        out = np.zeros(self.n_items, dtype=np.dtype(self._STATE))
        self._call("read", ctypes.c_void_p(stream), ctypes.c_void_p(out.ctypes.data))
        return out

    def reset(self, stream: int = 0) -> None:
        self._call("reset", ctypes.c_void_p(stream))

    def state_device_ptr(self) -> int:
        p = ctypes.c_void_p()
        self._call("state_device_ptr", ctypes.byref(p))
        return int(p.value)


def _item_check(prefix: str, what: str):
    """<what>_item_check(item): the status <prefix>_create would give this row"""
    def item_check(item) -> int:
        return int(getattr(load(), prefix + "_item_check")(ctypes.byref(item)))
    item_check.__name__ = item_check.__qualname__ = what + "_item_check"
    item_check.__doc__ = f"Status {prefix}_create would give this row (host arithmetic only: needs no device)."
    return item_check


def _dtype_of(struct):
    """<struct>_dtype(): the numpy structured dtype numpy derives from the ctypes structure, so the layout is stated once"""
    def dtype():
        import numpy as np
        return np.dtype(struct)
    dtype.__doc__ = f"numpy structured dtype with the layout of {struct.__doc__.split(':')[0]}."
    return dtype


batch_item_check = _item_check("cavmd_batch", "batch")
bussi_batch_item_check = _item_check("cavmd_bussi_batch", "bussi_batch")
recorder_item_check = _item_check("cavmd_recorder", "recorder")
field_item_check = _item_check("cavmd_field_recorder", "field")
verlet_item_check = _item_check("cavmd_verlet", "verlet")
bath_item_check = _item_check("cavmd_bath", "bath")
thermalize_item_check = _item_check("cavmd_thermalize", "thermalize")
ledger_item_check = _item_check("cavmd_ledger", "ledger")
draw_item_check = _item_check("cavmd_draw", "draw")
coulomb_item_check = _item_check("cavmd_coulomb", "coulomb")
trajectory_item_check = _item_check("cavmd_trajectory", "trajectory")

record_dtype = _dtype_of(Record)
field_record_dtype = _dtype_of(FieldRecord)
verlet_state_dtype = _dtype_of(VerletState)
bath_state_dtype = _dtype_of(BathState)
thermalize_state_dtype = _dtype_of(ThermalizeState)
ledger_row_dtype = _dtype_of(LedgerRow)
draw_state_dtype = _dtype_of(DrawState)
trajectory_header_dtype = _dtype_of(TrajectoryHeader)
snapshot_header_dtype = _dtype_of(SnapshotHeader)


class Batch(_ItemTableHandle):
    """Owns one cavmd_batch: B independent small systems evaluated by ONE kernel launch, one workgroup per system
    (the reference's replica loop, examples/05_advanced_run.py:1570-1612, on one GPU).  Launched by N descending."""
    _ITEM, _PREFIX = BatchItem, "cavmd_batch"
    _size = staticmethod(lambda it: int(it.N))

    def __init__(self, workspace: Workspace, items, history_depth: int = 64):
        self.history_depth = int(history_depth)
        self._create(workspace, items, self.history_depth)

    def compute(self, stream: int = 0) -> None:
        check(self._lib.cavmd_batch_compute(self._h, ctypes.c_void_p(stream)), "cavmd_batch_compute")

    def last_sequence(self) -> int:
        out = ctypes.c_uint64()
        check(self._lib.cavmd_batch_last_sequence(self._h, ctypes.byref(out)), "cavmd_batch_last_sequence")
        return int(out.value)

    def results(self):
        """The n_items result blocks of the last evaluation (a ctypes array of Result)."""
        out = (Result * self.n_items)()
        check(self._lib.cavmd_batch_results_read(self._h, out), "cavmd_batch_results_read")
        return out

    def results_at(self, sequence: int):
        out = (Result * self.n_items)()
        check(self._lib.cavmd_batch_results_at(self._h, int(sequence), out), "cavmd_batch_results_at")
        return out

    def energies_at(self, sequence: int):
        """(n_items, 3) array: harmonic, coupling, dipole-self energy of every system at evaluation `sequence`."""
        import numpy as np
        out = np.empty((self.n_items, 3), dtype=np.float64)
        check(self._lib.cavmd_batch_energies_at(self._h, int(sequence), ctypes.c_void_p(out.ctypes.data)),
              "cavmd_batch_energies_at")
        return out

    def results_device_ptr(self) -> int:
        p = ctypes.c_void_p()
        check(self._lib.cavmd_batch_results_device_ptr(self._h, ctypes.byref(p)), "cavmd_batch_results_device_ptr")
        return int(p.value)


SHARED_CAVITY_MAX_MEMBERS = 1024
shared_cavity_item_check = _item_check("cavmd_shared_cavity", "shared_cavity")


def shared_cavity_table_check(items):
    """(status, n_cavities) cavmd_shared_cavity_create would give this table (host arithmetic only: needs no device);
    n_cavities is None for a table that is refused."""
    items = list(items)
    n = ctypes.c_uint32()
    st = int(load().cavmd_shared_cavity_table_check(len(items), (SharedCavityItem * max(len(items), 1))(*items), ctypes.byref(n)))
    return st, (int(n.value) if st == CAVMD_OK else None)


class SharedCavity(_ItemTableHandle):
    """Owns one cavmd_shared_cavity: the items of a batch grouped into cavities, each cavity's photon coupled to the summed
    dipole of its members; TWO kernel launches per evaluation, one workgroup per item in each.  Launched by N descending."""
    _ITEM, _PREFIX = SharedCavityItem, "cavmd_shared_cavity"
    _size = staticmethod(lambda it: int(it.N))

    def __init__(self, workspace: Workspace, items):
        self._create(workspace, items)

    def compute(self, stream: int = 0) -> None:
        check(self._lib.cavmd_shared_cavity_compute(self._h, ctypes.c_void_p(stream)), "cavmd_shared_cavity_compute")

    def last_sequence(self) -> int:
        out = ctypes.c_uint64()
        self._call("last_sequence", ctypes.byref(out))
        return int(out.value)

    def results(self, stream: int = 0):
        """The n_items result blocks of the last evaluation (a ctypes array of Result), after a wait for ``stream``."""
        out = (Result * self.n_items)()
        self._call("results_read", ctypes.c_void_p(stream), out)
        return out

    def results_device_ptr(self) -> int:
        p = ctypes.c_void_p()
        self._call("results_device_ptr", ctypes.byref(p))
        return int(p.value)

    def cell_dipoles_device_ptr(self) -> int:
        p = ctypes.c_void_p()
        self._call("cell_dipoles_device_ptr", ctypes.byref(p))
        return int(p.value)

    def count(self) -> int:
        n = ctypes.c_uint32()
        self._call("count", ctypes.byref(n))
        return int(n.value)

    def carrier(self, cavity: int) -> int:
        item = ctypes.c_uint32()
        self._call("carrier", int(cavity), ctypes.byref(item))
        return int(item.value)


def bussi_batch_input_make(deltaT, set_T, tau, normal_variate, gamma_variate) -> BussiBatchInput:
    """One input row with the c = exp(-dt / tau) and the skip flag cavmd_bussi_step_device would use (host arithmetic)."""
    row = BussiBatchInput()
    check(load().cavmd_bussi_batch_input_make(float(deltaT), float(set_T), float(tau), float(normal_variate),
                                              float(gamma_variate), ctypes.byref(row)), "cavmd_bussi_batch_input_make")
    return row


class BussiBatch(_ItemTableHandle, _Snapshots):
    """Owns one cavmd_bussi_batch: the translational Bussi thermostat step of B independent small systems as ONE kernel
    launch, one workgroup per system, its per-step inputs read from device memory.  Launched by n_members descending."""
    _ITEM, _PREFIX = BussiBatchItem, "cavmd_bussi_batch"
    _size = staticmethod(lambda it: int(it.n_members))

    def __init__(self, workspace: Workspace, items):
        self._create(workspace, items)

    def step(self, stream: int, inputs_ptr: int) -> None:
        """One kernel: the step of every item, inputs read from the n_items device rows at `inputs_ptr` when the kernel runs."""
        check(self._lib.cavmd_bussi_batch_step(self._h, ctypes.c_void_p(stream), ctypes.c_void_p(inputs_ptr)),
              "cavmd_bussi_batch_step")

    def last_sequence(self) -> int:
        out = ctypes.c_uint64()
        check(self._lib.cavmd_bussi_batch_last_sequence(self._h, ctypes.byref(out)), "cavmd_bussi_batch_last_sequence")
        return int(out.value)

    def read(self, raise_refused: bool = True):
        """The n_items states after the last step (a ctypes array of BussiDeviceState).  A refusal since the last read raises
        CavmdError(CAVMD_ERR_BAD_PARAMS) once; with raise_refused=False it returns (states, refused_flag) instead."""
        out = (BussiDeviceState * self.n_items)()
        st = self._lib.cavmd_bussi_batch_read(self._h, out)
        if not raise_refused and st in (CAVMD_OK, CAVMD_ERR_BAD_PARAMS):
            return out, st == CAVMD_ERR_BAD_PARAMS
        check(st, "cavmd_bussi_batch_read")
        return out

    def reset(self, stream: int = 0) -> None:
        check(self._lib.cavmd_bussi_batch_reset(self._h, ctypes.c_void_p(stream)), "cavmd_bussi_batch_reset")

    def state_device_ptr(self) -> int:
        p = ctypes.c_void_p()
        check(self._lib.cavmd_bussi_batch_state_device_ptr(self._h, ctypes.byref(p)), "cavmd_bussi_batch_state_device_ptr")
        return int(p.value)


class Recorder(_SeriesHandle):
    """Owns one cavmd_recorder: the per-step observables of B independent small systems appended, by ONE kernel launch per
    call, to a time series in device memory whose write position lives on the device (a graph replay appends a new row).
    Launched by max(N, n_members) descending."""
    _ITEM, _PREFIX, _RECORD = RecorderItem, "cavmd_recorder", Record
    _size = staticmethod(lambda it: max(int(it.N), int(it.n_members)))

    def __init__(self, workspace: Workspace, items, capacity: int, period: int, kB: float):
        self.capacity, self.period, self.kB = int(capacity), int(period), float(kB)
        if self.capacity < 0 or self.period < 0:
            raise CavmdError(CAVMD_ERR_INVALID_VALUE, error_string(CAVMD_ERR_INVALID_VALUE), "cavmd_recorder_create")
        self._create(workspace, items, self.capacity, self.period, self.kB)

    def record(self, stream: int = 0) -> None:
        """One kernel: every item's call counter moves; on every period-th call the item appends one row."""
        check(self._lib.cavmd_recorder_record(self._h, ctypes.c_void_p(stream)), "cavmd_recorder_record")


class FieldRecorder(_SeriesHandle):
    """Owns one cavmd_field_recorder: rho(k) of B independent small systems, its correlation with each system's stored
    reference fields and the reference bookkeeping, appended by ONE kernel launch per call to a time series in device memory
    (a graph replay appends a new row and takes references when they are due).  Launched by N descending."""
    _ITEM, _PREFIX, _RECORD = FieldItem, "cavmd_field_recorder", FieldRecord
    _size = staticmethod(lambda it: int(it.N))

    def __init__(self, workspace: Workspace, items, wavevectors, capacity: int, period: int, max_references: int,
                 reference_interval: int):
        import numpy as np
        kv = np.ascontiguousarray(wavevectors, dtype=np.float64).reshape(-1, 3)
        self.n_k = int(kv.shape[0])
        self.capacity, self.period = int(capacity), int(period)
        self.max_references, self.reference_interval = int(max_references), int(reference_interval)
        if self.capacity < 0 or self.period < 0 or self.max_references < 0 or self.reference_interval < 0 \
                or self.max_references >= 2**32:
            raise CavmdError(CAVMD_ERR_INVALID_VALUE, error_string(CAVMD_ERR_INVALID_VALUE), "cavmd_field_recorder_create")
        self._create(workspace, items, self.n_k, ctypes.c_void_p(kv.ctypes.data), self.capacity, self.period,
                     self.max_references, self.reference_interval)

    def record(self, stream: int = 0, take_reference_ptr: int = 0) -> None:
        """One kernel: every item's call counter moves; on every period-th call the item appends one row.
        take_reference_ptr: 0 or the device address of n_items uint32 words read when the kernel runs."""
        check(self._lib.cavmd_field_recorder_record(self._h, ctypes.c_void_p(stream), ctypes.c_void_p(take_reference_ptr)),
              "cavmd_field_recorder_record")

    def set_time_rule(self, time0_ptr: int, stride_bytes: int, time_interval: float, reference_time_interval: float = 0.0) -> None:
        """Rows (and, with reference_time_interval > 0, references) by each item's own clock: the double at device address
        time0_ptr + item * stride_bytes.  time_interval 0 switches the rule off.  Set it before a capture."""
        check(self._lib.cavmd_runclock_field_set_rule(self._h, ctypes.c_void_p(int(time0_ptr)), int(stride_bytes),
                                                      float(time_interval), float(reference_time_interval)),
              "cavmd_runclock_field_set_rule")

    def read_fields(self, stream: int, item: int):
        """(rho_now, rho_refs, ref_rows) of one item after synchronising `stream`: complex arrays of shape (n_k,) and
        (n_refs, n_k), and the row each reference was taken at."""
        import numpy as np
        now = np.zeros(2 * self.n_k)
        refs = np.zeros((self.max_references, 2 * self.n_k))
        ref_rows = np.zeros(self.max_references, dtype=np.uint64)
        n = ctypes.c_uint32()
        check(self._lib.cavmd_field_recorder_read_fields(self._h, ctypes.c_void_p(stream), int(item),
                                                         ctypes.c_void_p(now.ctypes.data), ctypes.c_void_p(refs.ctypes.data),
                                                         ctypes.c_void_p(ref_rows.ctypes.data), ctypes.byref(n)),
              "cavmd_field_recorder_read_fields")
        return now.view(np.complex128), refs[:n.value].copy().view(np.complex128), ref_rows[:n.value].copy()


def verlet_input_make(dt, gamma=0.0, kT=0.0, uniform=(0.0, 0.0, 0.0)) -> VerletInput:
    """One input row with langevin_coeff = sqrt(6 gamma kT / dt) and the skip flag taken by the library (host arithmetic)."""
    row = VerletInput()
    u = (ctypes.c_double * 3)(*[float(x) for x in uniform])
    check(load().cavmd_verlet_input_make(float(dt), float(gamma), float(kT), ctypes.byref(u), ctypes.byref(row)),
          "cavmd_verlet_input_make")
    return row


class Verlet(_StateHandle):
    """Owns one cavmd_verlet: the two velocity-Verlet half-steps of B independent small systems, each ONE kernel launch, one
    workgroup per system, the step's inputs read from device memory.  Launched by N descending."""
    _ITEM, _PREFIX, _STATE = VerletItem, "cavmd_verlet", VerletState
    _size = staticmethod(lambda it: int(it.N))

    def __init__(self, workspace: Workspace, items):
        self._create(workspace, items)

    def accelerations(self, stream: int = 0) -> None:
        """One kernel: a = F / m (and the net force) of every item from the force arrays as they are."""
        check(self._lib.cavmd_verlet_accelerations(self._h, ctypes.c_void_p(stream)), "cavmd_verlet_accelerations")

    def step_one(self, stream: int, inputs_ptr: int) -> None:
        """One kernel: kick, drift and wrap of every item, inputs read from the n_items device rows when the kernel runs."""
        check(self._lib.cavmd_verlet_step_one(self._h, ctypes.c_void_p(stream), ctypes.c_void_p(inputs_ptr)),
              "cavmd_verlet_step_one")

    def step_two(self, stream: int, inputs_ptr: int) -> None:
        """One kernel: net force, Langevin bath of the one coupled particle, acceleration and kick of every item."""
        check(self._lib.cavmd_verlet_step_two(self._h, ctypes.c_void_p(stream), ctypes.c_void_p(inputs_ptr)),
              "cavmd_verlet_step_two")

    def kick(self, stream: int, inputs_ptr: int, forces_ptr: int, weight: float) -> None:
        """One kernel: v += (f / m) (weight dt) of every item, f through the DEVICE table of n_items device pointers at
        ``forces_ptr``, read with the input rows when the kernel runs.  Nothing but the velocities is written."""
        check(self._lib.cavmd_mts_verlet_kick(self._h, ctypes.c_void_p(stream), ctypes.c_void_p(inputs_ptr), ctypes.c_void_p(forces_ptr),
                                          float(weight)), "cavmd_mts_verlet_kick")


BATH_KEY_STRIDE = 0x9E3779B97F4A7C15


def bath_item_key(seed: int, i: int) -> int:
    """The Philox key of item i under the object's seed: (seed + 0x9E3779B97F4A7C15 * (i + 1)) mod 2^64.  The stride is odd, so
    the keys of 2^64 consecutive items are distinct."""
    return (int(seed) + BATH_KEY_STRIDE * (int(i) + 1)) & 0xFFFFFFFFFFFFFFFF


class Bath(_StateHandle):
    """Owns one cavmd_bath: the second half-step of an integrator batch with a Langevin bath on any set of particles of every
    system, ONE kernel launch, the 3 N variates drawn inside it.  Created from a ``Verlet`` (kept alive here, with its
    workspace) and closed before it; launched in the integrator's order."""
    _ITEM, _PREFIX, _STATE = BathItem, "cavmd_bath", BathState
    _DEFERRED = "_deferred_baths"                 # emptied before the integrators among _deferred_children
    _size = staticmethod(lambda it: int(it.N))

    def __init__(self, verlet: "Verlet", items):
        if verlet is None or not getattr(verlet, "_h", None) or not verlet._h.value:
            raise CavmdError(CAVMD_ERR_INVALID_VALUE, error_string(CAVMD_ERR_INVALID_VALUE), "cavmd_bath_create")
        self._create(verlet, items)               # cavmd_bath_create(integrator, n_items, items, &handle)
        self._verlet, self._ws = verlet, verlet._ws

    def step_two(self, stream: int, inputs_ptr: int) -> None:
        """One kernel, in place of ``Verlet.step_two``: net force, the row's and the group's baths, acceleration and kick."""
        check(self._lib.cavmd_bath_step_two(self._h, ctypes.c_void_p(stream), ctypes.c_void_p(inputs_ptr)), "cavmd_bath_step_two")


class Thermalize(_StateHandle):
    """Owns one cavmd_thermalize: the start of B independent small systems, ONE kernel launch, one workgroup per system: seeded
    Maxwell-Boltzmann velocities on any set of particles, their momentum taken out, the photon's velocity and placement.
    Launched by N descending."""
    _ITEM, _PREFIX, _STATE = ThermalizeItem, "cavmd_thermalize", ThermalizeState
    _size = staticmethod(lambda it: int(it.N))

    def __init__(self, workspace: Workspace, items):
        self._create(workspace, items)

    def run(self, stream: int = 0) -> None:
        """One kernel: the velocities, counters and photon of every item."""
        check(self._lib.cavmd_thermalize_run(self._h, ctypes.c_void_p(stream)), "cavmd_thermalize_run")


class Ledger(_SeriesHandle):
    """Owns one cavmd_ledger: every term of the conserved energy of B independent small systems appended, by ONE kernel launch
    per call, to a time series in device memory whose write position lives on the device (a graph replay appends a new row).
    Launched by max(N, n_members) descending."""
    _ITEM, _PREFIX, _RECORD = LedgerItem, "cavmd_ledger", LedgerRow
    _size = staticmethod(lambda it: max(int(it.N), int(it.n_members)))

    def __init__(self, workspace: Workspace, items, capacity: int, period: int, kB: float):
        self.capacity, self.period, self.kB = int(capacity), int(period), float(kB)
        if self.capacity < 0 or self.period < 0:
            raise CavmdError(CAVMD_ERR_INVALID_VALUE, error_string(CAVMD_ERR_INVALID_VALUE), "cavmd_ledger_create")
        self._create(workspace, items, self.capacity, self.period, self.kB)

    def record(self, stream: int = 0) -> None:
        """One kernel: every item's call counter moves; on every period-th call the item appends one row."""
        check(self._lib.cavmd_ledger_record(self._h, ctypes.c_void_p(stream)), "cavmd_ledger_record")

    def set_time_rule(self, time_interval: float, max_time: float = 0.0) -> None:
        """Rows by each item's own clock (``d_time``): a row where the clock moved by time_interval since the item's last
        one, none past max_time (0: no last time).  time_interval 0 switches the rule off.  Set it before a capture."""
        check(self._lib.cavmd_runclock_ledger_set_rule(self._h, float(time_interval), float(max_time)),
              "cavmd_runclock_ledger_set_rule")


class Draw(_StateHandle):
    """Owns one cavmd_draw: the integrator's and the thermostat's input rows of B independent small systems written by ONE
    kernel launch per step, one lane per system, from a seeded counter-based generator, with the step's dt (fixed, or the
    adaptive rule on the recorder's last row).  Items cost the same: launched in item order."""
    _ITEM, _PREFIX, _STATE = DrawItem, "cavmd_draw", DrawState
    _size = staticmethod(lambda it: 0)

    def __init__(self, workspace: Workspace, seed: int, items):
        self.seed = int(seed)
        if not 0 <= self.seed < 2**64:
            raise CavmdError(CAVMD_ERR_INVALID_VALUE, error_string(CAVMD_ERR_INVALID_VALUE), "cavmd_draw_create")
        self._create(workspace, items, before=(self.seed,))

    def fill(self, stream: int = 0) -> None:
        """One kernel: both input rows, the counters and the dt of every item."""
        check(self._lib.cavmd_draw_fill(self._h, ctypes.c_void_p(stream)), "cavmd_draw_fill")

    def set_end(self, first: int, t_end) -> None:
        """End times of items first .. first + len(t_end) - 1 (0: none); an item whose ``elapsed`` has reached its own rests."""
        values = [float(t) for t in t_end]
        check(self._lib.cavmd_runclock_draw_set_end(self._h, int(first), len(values), (ctypes.c_double * max(len(values), 1))(*values)),
              "cavmd_runclock_draw_set_end")

    def finished(self, stream: int = 0) -> int:
        """How many items rest behind their end time, after synchronising `stream`."""
        n = ctypes.c_uint64()
        check(self._lib.cavmd_runclock_draw_finished(self._h, ctypes.c_void_p(stream), ctypes.byref(n)), "cavmd_runclock_draw_finished")
        return int(n.value)


def molecular_order(lib=None):
    """(ROWS, S): the particles a workgroup of the molecular force kernel owns and the partial sums per particle, as the
    library was compiled (S = CAVMD_MOLECULAR_J_SPLIT fixes the published summation order)."""
    rows, split = ctypes.c_int(), ctypes.c_int()
    check((lib or load()).cavmd_molecular_order(ctypes.byref(rows), ctypes.byref(split)), "cavmd_molecular_order")
    return int(rows.value), int(split.value)


def molecular_pair_make(epsilon, sigma, r_cut, shift=True) -> MolecularPair:
    """One entry of the pair table with the constants taken by the library (host arithmetic)."""
    out = MolecularPair()
    check(load().cavmd_molecular_pair_make(float(epsilon), float(sigma), float(r_cut), 1 if shift else 0, ctypes.byref(out)),
          "cavmd_molecular_pair_make")
    return out


def molecular_params(n_types, harmonic, lj, shift=True) -> MolecularParams:
    """harmonic: {bond type: (K, r0)}; lj: {(type a, type b): (epsilon, sigma, r_cut)}, entered symmetrically; type pairs that
    are not listed keep rcutsq = 0 and do not interact."""
    prm = MolecularParams()
    prm.n_types = int(n_types)
    prm.n_bond_types = (max(int(t) for t in harmonic) + 1) if harmonic else 0
    for t, (K, r0) in harmonic.items():
        if not 0 <= int(t) < 8:
            raise ValueError("bond types are 0 .. 7")
        prm.bond[int(t)].K, prm.bond[int(t)].r0 = float(K), float(r0)
    for (a, b), (epsilon, sigma, r_cut) in lj.items():
        if not (0 <= int(a) < 8 and 0 <= int(b) < 8):
            raise ValueError("particle types are 0 .. 7")
        pair = molecular_pair_make(epsilon, sigma, r_cut, shift)
        prm.pair[int(a)][int(b)] = pair
        prm.pair[int(b)][int(a)] = pair
    return prm


def molecular_params_check(params: MolecularParams) -> int:
    return int(load().cavmd_molecular_params_check(ctypes.byref(params)))


def molecular_item_check(params: MolecularParams, item: MolecularItem) -> int:
    """Status cavmd_molecular_create would give this row (host arithmetic only: needs no device)."""
    return int(load().cavmd_molecular_item_check(ctypes.byref(params), ctypes.byref(item)))


class Molecular(_ItemTableHandle):
    """Owns one cavmd_molecular: the harmonic bonds and Lennard-Jones pairs of B independent small systems in ONE kernel
    launch, ceil(N / ROWS) workgroups per system, all pairs out of LDS.  Workgroups start by N descending."""
    _ITEM, _PREFIX = MolecularItem, "cavmd_molecular"
    _size = staticmethod(lambda it: int(it.N))

    def __init__(self, workspace: Workspace, params: MolecularParams, items):
        self.params = params
        self._create(workspace, items, before=(ctypes.byref(params),))

    def compute(self, stream: int = 0) -> None:
        """One kernel: every entry of every item's force array."""
        check(self._lib.cavmd_molecular_compute(self._h, ctypes.c_void_p(stream)), "cavmd_molecular_compute")


def coulomb_order(lib=None):
    """(ROWS, S, KROWS, T): the particles a workgroup of the Coulomb force kernel owns and the lanes that share one, the
    k-vectors a workgroup of the structure-factor kernel owns and the lanes that share one, as the library was compiled."""
    v = [ctypes.c_int() for _ in range(4)]
    check((lib or load()).cavmd_coulomb_order(*[ctypes.byref(x) for x in v]), "cavmd_coulomb_order")
    return tuple(int(x.value) for x in v)


def coulomb_parameters(r_cut, accuracy):
    """(kappa, k_cut) = (sqrt(-ln accuracy) / r_cut, 2 kappa sqrt(-ln accuracy)) (host arithmetic)."""
    kappa, k_cut = ctypes.c_double(), ctypes.c_double()
    check(load().cavmd_coulomb_parameters(float(r_cut), float(accuracy), ctypes.byref(kappa), ctypes.byref(k_cut)),
          "cavmd_coulomb_parameters")
    return float(kappa.value), float(k_cut.value)


def coulomb_k_count(item: CoulombItem) -> int:
    """K, the kept k-vectors of an item the library accepts; raises CavmdError otherwise."""
    K = ctypes.c_uint32()
    check(load().cavmd_coulomb_k_count(ctypes.byref(item), ctypes.byref(K)), "cavmd_coulomb_k_count")
    return int(K.value)


def ewald_order(lib=None):
    """(TILE, SEG, MAX_M, ROWS, SEGROWS) of the factored reciprocal method: the particles whose phase tables launch 1 holds in
    LDS at a time, the k-vectors of a segment, the largest |m| per axis, the particles a workgroup of launch 2 owns and the
    segments a workgroup of launch 1 owns, as the library was compiled."""
    v = [ctypes.c_int() for _ in range(5)]
    check((lib or load()).cavmd_ewald_order(*[ctypes.byref(x) for x in v]), "cavmd_ewald_order")
    return tuple(int(x.value) for x in v)


class Coulomb(_ItemTableHandle):
    """Owns one cavmd_coulomb: the Ewald Coulomb forces of B independent small systems in TWO kernel launches (structure
    factors, ceil(K / KROWS) workgroups per system; forces, ceil(N / ROWS)).  Workgroups start by N descending."""
    _ITEM, _PREFIX = CoulombItem, "cavmd_coulomb"
    _size = staticmethod(lambda it: int(it.N))

    def __init__(self, workspace: Workspace, items):
        self._create(workspace, items)

    def compute(self, stream: int = 0) -> None:
        """Two kernels: every structure factor, then every entry of every item's force array."""
        check(self._lib.cavmd_coulomb_compute(self._h, ctypes.c_void_p(stream)), "cavmd_coulomb_compute")

    def set_long_forces(self, long_ptrs) -> None:
        """Gives every item its LONG array (device addresses, 0 for an item with N == 0), or drops the split (all 0)."""
        ptrs = [int(p) for p in long_ptrs]
        arr = (ctypes.c_void_p * max(len(ptrs), 1))(*ptrs)
        check(self._lib.cavmd_mts_coulomb_set_long_forces(self._h, len(ptrs), arr), "cavmd_mts_coulomb_set_long_forces")

    def compute_parts(self, stream: int = 0, parts: int = COULOMB_PART_SHORT | COULOMB_PART_LONG) -> None:
        """SHORT: one kernel into the items' force arrays; LONG: two kernels into their long arrays; both: three."""
        check(self._lib.cavmd_mts_coulomb_compute_parts(self._h, ctypes.c_void_p(stream), int(parts)), "cavmd_mts_coulomb_compute_parts")

    def set_reciprocal(self, method: int) -> None:
        """Which two kernels ``compute`` enqueues from now on: EWALD_RECIPROCAL_DIRECT or EWALD_RECIPROCAL_FACTORED.  Raises
        CavmdError (CAVMD_ERR_CAPACITY, nothing changed) when an item's largest |m| exceeds the factored method's limit."""
        check(self._lib.cavmd_ewald_set_reciprocal(self._h, int(method)), "cavmd_ewald_set_reciprocal")

    @property
    def reciprocal(self) -> int:
        method = ctypes.c_int()
        check(self._lib.cavmd_ewald_get_reciprocal(self._h, ctypes.byref(method)), "cavmd_ewald_get_reciprocal")
        return int(method.value)

    def structure_device_ptr(self):
        """(device address of the structure-factor table, per-item offsets in entries of two doubles): item i owns K_i + 1
        entries, {A, B} per k-vector and then {Q, 0}.  Valid until the next set_items / close."""
        p, off = ctypes.c_void_p(), ctypes.POINTER(ctypes.c_uint32)()
        check(self._lib.cavmd_coulomb_structure_device_ptr(self._h, ctypes.byref(p), ctypes.byref(off)),
              "cavmd_coulomb_structure_device_ptr")
        return int(p.value), [int(off[i]) for i in range(self.n_items)]


def trajectory_layout(max_N: int, format: int) -> TrajectoryLayout:
    """Where the sections of a frame of up to max_N particles lie (host arithmetic); raises CavmdError where the library
    refuses."""
    out = TrajectoryLayout()
    check(load().cavmd_trajectory_layout(int(max_N), int(format), ctypes.byref(out)), "cavmd_trajectory_layout")
    return out


def trajectory_frame_dtype(layout: TrajectoryLayout):
    """numpy structured dtype of one frame: the header's columns at their offsets, then ``position`` and ``velocity`` as
    (max_N, 3) float64 or float32 and ``image`` as (max_N, 3) int32 at the layout's offsets, itemsize frame_bytes."""
    import numpy as np
    head = np.dtype(TrajectoryHeader)
    names, formats, offsets = list(head.names), [head.fields[n][0] for n in head.names], [head.fields[n][1] for n in head.names]
    element = np.dtype("<f8") if layout.format == TRAJECTORY_F64 else np.dtype("<f4")
    for name, fmt, off in (("position", element, layout.position_offset), ("velocity", element, layout.velocity_offset),
                           ("image", np.dtype("<i4"), layout.image_offset)):
        names.append(name)
        formats.append(np.dtype((fmt, (int(layout.max_N), 3))))
        offsets.append(int(off))
    return np.dtype({"names": names, "formats": formats, "offsets": offsets, "itemsize": int(layout.frame_bytes)})


class Trajectory(_SeriesHandle):
    """Owns one cavmd_trajectory: frames of the positions, velocities and images of B independent small systems appended, by
    ONE kernel launch per call, to a ring in device memory; whether a call writes a frame is decided on the device (a graph
    replay records when a frame is due).  Launched by N descending."""
    _ITEM, _PREFIX, _RECORD = TrajectoryItem, "cavmd_trajectory", None
    _size = staticmethod(lambda it: int(it.N))

    def __init__(self, workspace: Workspace, items, max_N: int, format: int, capacity: int, period: int = 1,
                 time_interval: float = 0.0):
        self.capacity, self.period, self.time_interval = int(capacity), int(period), float(time_interval)
        self.max_N, self.format = int(max_N), int(format)
        if self.capacity < 0 or self.period < 0 or not 0 <= self.max_N < 2**32 or not 0 <= self.format < 2**32:
            raise CavmdError(CAVMD_ERR_INVALID_VALUE, error_string(CAVMD_ERR_INVALID_VALUE), "cavmd_trajectory_create")
        self._create(workspace, items, self.max_N, self.format, self.capacity, self.period, self.time_interval)
        self.layout = trajectory_layout(self.max_N, self.format)
        self._RECORD = trajectory_frame_dtype(self.layout)   # what _SeriesHandle.read allocates: whole frames

    def record(self, stream: int = 0, take_frame_ptr: int = 0) -> None:
        """One kernel: every item's call counter moves; an item whose frame is due (or whose take word is set) appends one.
        take_frame_ptr: 0 or the device address of n_items uint32 words read when the kernel runs."""
        check(self._lib.cavmd_trajectory_record(self._h, ctypes.c_void_p(stream), ctypes.c_void_p(take_frame_ptr)),
              "cavmd_trajectory_record")
