"""cavitymd -- MI355X-native cavity-MD force engine (the cavity-force hot path of
muhammadhasyim/cav-hoomd behind the same Python surface).

Installed into a HOOMD-blue tree this package takes the place of ``hoomd.cavitymd`` for the cavity
force; standalone (no HOOMD, as in the build/test image) it is imported as ``cavitymd`` from the
``cav-hoomd_amd/`` directory.

    from cavitymd import CavityForce, PhysicalConstants, unwrap_positions
"""
from .utils import PhysicalConstants, unwrap_positions
from .forces import CavityForce
from .compute import CavityForceComputeHIP
from .history import EnergyHistory
from .batch import BatchEnergyHistory, CavityForceBatch
from .shared_cavity import SharedCavityForceBatch
from .thermostat_batch import BussiReservoirBatch
from .recorder import BatchRecorder
from .field_recorder import BatchFieldRecorder
from .integrator_batch import VerletBatch
from .step_draw import StepDraw
from .bath_batch import LangevinBathBatch
from .thermalize_batch import BatchThermalizer
from .ledger import BatchEnergyLedger
from .trajectory import BatchTrajectoryRecorder
from .checkpoint import BatchCheckpoint
from .run_clock import run_until_finished
from .molecular_batch import MolecularForceBatch
from .coulomb_batch import CoulombForceBatch
from .state import BoxDim, ParticleData, SystemDefinition
from . import _capi, bath_batch, checkpoint, coulomb_batch, field_recorder, integrator_batch, ledger, molecular_batch, observables, recorder, replicas, run_clock, shared_cavity, step_draw, synthetic, thermalize_batch, thermostat_batch, thermostats, trajectory

__all__ = [
    "CavityForce", "CavityForceComputeHIP", "CavityForceBatch", "SharedCavityForceBatch", "BatchEnergyHistory", "BussiReservoirBatch", "BatchRecorder", "BatchFieldRecorder", "VerletBatch", "StepDraw", "LangevinBathBatch", "BatchThermalizer", "BatchEnergyLedger", "BatchTrajectoryRecorder", "BatchCheckpoint", "run_until_finished", "MolecularForceBatch", "CoulombForceBatch", "EnergyHistory", "PhysicalConstants", "unwrap_positions", "BoxDim", "ParticleData",
    "SystemDefinition", "bath_batch", "checkpoint", "coulomb_batch", "field_recorder", "integrator_batch", "ledger", "molecular_batch", "observables", "recorder", "replicas", "run_clock", "shared_cavity", "step_draw", "synthetic", "thermalize_batch", "thermostat_batch", "thermostats", "trajectory",
]
__version__ = "0.1.0"
