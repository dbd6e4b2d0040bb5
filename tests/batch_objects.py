"""The eleven batch objects of include/cavmd.h, one table and one implementation of each check a machine WITHOUT a GPU can make
on all of them: the header declares and both libraries export each object's entry points and nothing stray, a C99 caller
compiles, links and runs, the layouts agree between the C compiler, ctypes and numpy, null arguments are refused, the launch
order is a stable descending sort, the Python class is exported and refuses CPU tensors, and a deferred destroy takes the
object before its workspace.  tests/test_batch_objects_abi.py runs every check on every row; the per-object tests/test_*_abi.py
call the same functions with their own row.  pytest does not rewrite the asserts of a module that is no test module, so each
assert here says what it found."""
import ctypes
import random
import re
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import abi_support as abi

byref, vp = ctypes.byref, ctypes.c_void_p
KB = 3.167e-6
_K_VECTOR = np.zeros((1, 3))


class NoBatch:
    """stands in for a force batch that is never looked at: the CPU tensor is refused first"""

    def __len__(self):
        return 1


class NoIntegrator:
    """stands in for an integrator that is never looked at: the CPU tensor is refused first"""
    n_systems = 1


def _cpu_system(cavitymd, cfg):
    pd = cavitymd.ParticleData.from_arrays(cfg["position"], cfg["typeid"], cfg["charge"], cfg["image"], cfg["types"], cfg["box"],
                                           device="cpu")
    return cavitymd.SystemDefinition(pd)


def _lattice(cavitymd):
    from cavitymd import synthetic
    cfg = synthetic.diatomic_lattice(2, 8.0, seed=3)
    return (_cpu_system(cavitymd, cfg),) + synthetic.diatomic_bonds(cfg)


def _batch_on_cpu(cavitymd):
    from cavitymd import synthetic
    cfg = synthetic.config1()
    return [lambda: cavitymd.CavityForceBatch([_cpu_system(cavitymd, cfg)], cfg["params"])]


def _bussi_batch_on_cpu(cavitymd):
    return [lambda: cavitymd.BussiReservoirBatch(kT=1.0, tau=0.5).attach([torch.zeros((10, 4), dtype=torch.float64)], 27.0)]


def _recorder_on_cpu(cavitymd):
    vel = torch.zeros((10, 4), dtype=torch.float64)
    return [lambda: cavitymd.BatchRecorder(NoBatch(), [vel]),
            lambda: cavitymd.BatchRecorder(NoBatch(), [None], net_forces=[vel]),
            lambda: cavitymd.BatchRecorder(NoBatch(), [np.zeros((10, 4))])]


def _field_recorder_on_cpu(cavitymd):
    return [lambda: cavitymd.BatchFieldRecorder([torch.zeros((10, 3), dtype=torch.float64)]),
            lambda: cavitymd.BatchFieldRecorder([np.zeros((10, 4))])]


def _verlet_on_cpu(cavitymd):
    return [lambda: cavitymd.VerletBatch(NoBatch(), [torch.zeros((10, 4), dtype=torch.float64)]),
            lambda: cavitymd.VerletBatch(NoBatch(), [np.zeros((10, 4))])]


def _bath_on_cpu(cavitymd):
    return [lambda: cavitymd.LangevinBathBatch(NoIntegrator(), [torch.zeros(10, dtype=torch.float64)], 1.0, 3),
            lambda: cavitymd.LangevinBathBatch(NoIntegrator(), [None, np.zeros(10)], 1.0, 3)]


def _ledger_on_cpu(cavitymd):
    vel = torch.zeros((10, 4), dtype=torch.float64)
    return [lambda: cavitymd.BatchEnergyLedger(NoBatch(), [vel]),
            lambda: cavitymd.BatchEnergyLedger(None, [vel]),
            lambda: cavitymd.BatchEnergyLedger(None, [None], terms=[[vel]]),
            lambda: cavitymd.BatchEnergyLedger(None, [np.zeros((10, 4))])]


def _thermalize_on_cpu(cavitymd):
    vel = torch.zeros((10, 4), dtype=torch.float64)
    return [lambda: cavitymd.BatchThermalizer([vel], 1.0, 3),
            lambda: cavitymd.BatchThermalizer([vel], 1.0, 3, cavity=NoBatch(), place_photon=True),
            lambda: cavitymd.BatchThermalizer([np.zeros((10, 4))], 1.0)]


def _draw_on_cpu(cavitymd):
    rows = torch.zeros((3, 8), dtype=torch.float64)
    return [lambda: cavitymd.StepDraw(1, integrator=rows, dt=1.0),
            lambda: cavitymd.StepDraw(1, thermostat=rows, set_T=1.0, tau=1.0, dof=3.0, dt=1.0),
            lambda: cavitymd.StepDraw(1, integrator=np.zeros((3, 8)), dt=1.0)]


def _molecular_on_cpu(cavitymd):
    sysdef, bonds, bond_typeid = _lattice(cavitymd)
    return [lambda: cavitymd.MolecularForceBatch([sysdef], [bonds], [bond_typeid], harmonic={0: dict(k=1.0, r0=2.0)},
                                                 lj={("O", "O"): dict(epsilon=1e-4, sigma=6.0, r_cut=8.0)})]


def _coulomb_on_cpu(cavitymd):
    sysdef, bonds, _ = _lattice(cavitymd)
    return [lambda: cavitymd.CoulombForceBatch([sysdef], [bonds], r_cut=6.0, accuracy=1e-6)]


def _row(name, skip=None, **kw):
    return SimpleNamespace(name=name, prefix="cavmd_" + name, typedef="cavmd_" + name, destroy="cavmd_%s_destroy" % name,
                           program=name + "_abi_check", ok=name.upper().replace("_", "-") + "-ABI-OK", skip=skip or {}, **kw)


# One row per object, in the header's order (as _capi._PROTOTYPES is).  entry_points is spelled out: derived from the header or from _capi._PROTOTYPES it would check nothing.
#   structs      which -> (ctypes structure, sizeof, {field: offset} pinned as literals); `which` is the C program's name for it
#   dtypes       which -> the _capi function giving the numpy dtype of that structure
#   no_device    the line the C program prints where cavmd_create finds no device
#   create       (capi, item) -> what cavmd_<name>_create takes between the workspace (for the bath: the integrator) and the
#                out pointer
#   with_handle  (capi, item) -> {entry point: what it takes after the handle}; the rest of entry_points is without_handle
#   on_cpu       cavitymd -> constructor calls with CPU tensors, each of which must raise "no CPU fallback"
#   skip         {check letter: one-line reason} for a check that cannot apply to the object by its nature (none today)
OBJECTS = [
    _row("batch",
         entry_points=("item_check", "create", "destroy", "set_items", "compute", "last_sequence", "results_read", "results_at",
                       "energies_at", "results_device_ptr"),
         kernels=(b"cavity_batch_kernel",), no_device="no device: no workspace, hence no batch",
         structs={"item": ("BatchItem", 128, dict(d_pos=0, d_charge=8, d_image=16, d_force=24, Lx=32, Ly=40, Lz=48, params=56, N=88,
                                                  L_typeid=92, reserved=96)),
                  "params": ("Params", 32, {})},
         dtypes={}, good=abi.good_batch, without_handle=("item_check",),
         create=lambda capi, it: (1, byref(it), 4),
         with_handle=lambda capi, it: {"set_items": (0, 1, byref(it)), "compute": (None,),
                                       "last_sequence": (byref(ctypes.c_uint64()),), "results_read": (byref(capi.Result()),),
                                       "results_at": (1, byref(capi.Result())), "energies_at": (1, None),
                                       "results_device_ptr": (byref(vp()),)},
         handle="Batch", handle_methods=("compute", "last_sequence", "results", "results_at", "energies_at", "set_items", "close"),
         cls="CavityForceBatch", module="batch", methods=("compute", "energies", "energies_at", "history", "refresh", "last_sequence"),
         properties=("forces",), on_cpu=_batch_on_cpu),
    _row("bussi_batch",
         entry_points=("item_check", "input_make", "create", "destroy", "set_items", "step", "last_sequence", "read", "reset",
                       "state_device_ptr"),
         kernels=(b"bussi_batch_kernel",), no_device="no device: no workspace, hence no batch",
         structs={"item": ("BussiBatchItem", 64, dict(d_vel=0, d_members=8, n_members=16, reserved0=20, dof_translational=24,
                                                      reserved=32)),
                  "input": ("BussiBatchInput", 64, dict(normal_variate=0, gamma_variate=8, c=16, set_T=24, skip=32, reserved=40)),
                  "state": ("BussiDeviceState", 48, {})},
         dtypes={}, good=abi.good_bussi_batch, without_handle=("item_check", "input_make"),
         create=lambda capi, it: (1, byref(it)),
         with_handle=lambda capi, it: {"set_items": (0, 1, byref(it)), "step": (None, vp(0x1000)),
                                       "last_sequence": (byref(ctypes.c_uint64()),), "read": (byref(capi.BussiDeviceState()),),
                                       "reset": (None,), "state_device_ptr": (byref(vp()),)},
         handle="BussiBatch", handle_methods=("step", "read", "reset", "set_items", "last_sequence", "state_device_ptr", "close"),
         cls="BussiReservoirBatch", module="thermostat_batch",
         methods=("attach", "set_inputs", "draw_inputs", "step_async", "device_state", "reset_reservoir_energy"),
         properties=("reservoir_energy_translational", "reservoir_energy_rotational", "total_reservoir_energy",
                     "instantaneous_reservoir_translational", "instantaneous_reservoir_rotational",
                     "instantaneous_reservoir_total"),
         on_cpu=_bussi_batch_on_cpu),
    _row("recorder",
         entry_points=("item_check", "create", "destroy", "set_items", "record", "rows", "read", "reset", "device_ptr"),
         kernels=(b"recorder_batch_kernel",), no_device="no device: no workspace, hence no recorder",
         structs={"record": ("Record", 128, dict(call=0, eval_sequence=8, energy=16, total_dipole=40, q=64, cavity_kinetic=88,
                                                 cavity_temperature=96, kinetic_energy=104, force_mass_sum=112, reserved=120)),
                  "item": ("RecorderItem", 64, dict(d_result=0, d_vel=8, d_net_force=16, d_members=24, N=32, n_members=36,
                                                    reserved=40))},
         dtypes={"record": "record_dtype"}, good=abi.good_recorder, without_handle=("item_check",),
         create=lambda capi, it: (1, byref(it), 8, 1, KB),
         with_handle=lambda capi, it: {"set_items": (0, 1, byref(it)), "record": (None,),
                                       "rows": (None, byref(ctypes.c_uint64())), "read": (None, 0, 1, 0, 1, byref(capi.Record())),
                                       "reset": (None,), "device_ptr": (byref(vp()), byref(vp()))},
         handle="Recorder", handle_methods=("record", "rows", "read", "reset", "set_items", "device_ptr", "close"),
         cls="BatchRecorder", module="recorder", methods=("record", "rows", "read", "reset", "close"), properties=(),
         on_cpu=_recorder_on_cpu),
    _row("field_recorder",
         entry_points=("item_check", "create", "destroy", "set_items", "record", "rows", "read", "read_fields", "reset",
                       "device_ptr"),
         kernels=(b"field_recorder_batch_kernel",), no_device="no device: no workspace, hence no field recorder",
         structs={"record": ("FieldRecord", 160, dict(call=0, n_references=8, took_reference=12, rho2=16, reserved=24, F=32)),
                  "item": ("FieldItem", 64, dict(d_position=0, position_stride=8, N=16, reserved0=20, reserved=24))},
         dtypes={"record": "field_record_dtype"}, good=abi.good_field_recorder, without_handle=("item_check",),
         create=lambda capi, it: (1, byref(it), 1, vp(_K_VECTOR.ctypes.data), 8, 1, 1, 0),
         with_handle=lambda capi, it: {"set_items": (0, 1, byref(it)), "record": (None, None),
                                       "rows": (None, byref(ctypes.c_uint64())),
                                       "read": (None, 0, 1, 0, 1, byref(capi.FieldRecord())),
                                       "read_fields": (None, 0, None, None, None, byref(ctypes.c_uint32())), "reset": (None,),
                                       "device_ptr": (byref(vp()), byref(vp()))},
         handle="FieldRecorder", handle_methods=("record", "rows", "read", "read_fields", "reset", "set_items", "device_ptr", "close"),
         cls="BatchFieldRecorder", module="field_recorder", methods=("record", "rows", "read", "fields", "reset", "close"),
         properties=(), on_cpu=_field_recorder_on_cpu),
    _row("verlet",
         entry_points=("item_check", "input_make", "create", "destroy", "set_items", "accelerations", "step_one", "step_two", "read",
                       "reset", "state_device_ptr"),
         kernels=(b"verlet_step_one_kernel", b"verlet_step_two_kernel"),
         no_device="no device: no workspace, hence no integrator batch",
         structs={"item": ("VerletItem", 128, dict(d_force=32, N=96)), "input": ("VerletInput", 64, dict(skip=48)),
                  "state": ("VerletState", 32, {})},
         dtypes={"state": "verlet_state_dtype"}, good=abi.good_verlet, without_handle=("item_check", "input_make"),
         create=lambda capi, it: (1, byref(it)),
         with_handle=lambda capi, it: {"set_items": (0, 1, byref(it)), "accelerations": (None,), "step_one": (None, vp(0x1000)),
                                       "step_two": (None, vp(0x1000)), "read": (None, byref(capi.VerletState())),
                                       "reset": (None,), "state_device_ptr": (byref(vp()),)},
         handle="Verlet", handle_methods=("accelerations", "step_one", "step_two", "read", "reset", "set_items", "state_device_ptr",
                                          "close"),
         cls="VerletBatch", module="integrator_batch",
         methods=("set_inputs", "draw_inputs", "prime", "step_one", "step_two", "state", "reset", "close"), properties=(),
         on_cpu=_verlet_on_cpu),
    _row("bath",
         entry_points=("item_check", "create", "destroy", "set_items", "step_two", "read", "reset", "state_device_ptr"),
         kernels=(b"verlet_step_two_bath_kernel",), no_device="no device: no workspace, hence no integrator and no bath",
         structs={"item": ("BathItem", 64, dict(d_gamma=0, seed=8, kT=16, N=24, reserved0=28, reserved=32)),
                  "state": ("BathState", 32, dict(draws=0, coupled=8, reservoir=16, reserved=24))},
         dtypes={"state": "bath_state_dtype"}, good=abi.good_bath, without_handle=("item_check",),
         create=lambda capi, it: (1, byref(it)),
         with_handle=lambda capi, it: {"set_items": (0, 1, byref(it)), "step_two": (None, vp(0x1000)),
                                       "read": (None, byref(capi.BathState())), "reset": (None,),
                                       "state_device_ptr": (byref(vp()),)},
         handle="Bath", handle_methods=("step_two", "read", "reset", "set_items", "state_device_ptr", "close"),
         cls="LangevinBathBatch", module="bath_batch", methods=("step_two", "state", "reset", "close", "set_gammas"),
         properties=("bath",), on_cpu=_bath_on_cpu),
    _row("ledger",
         entry_points=("item_check", "create", "destroy", "set_items", "record", "rows", "read", "reset", "device_ptr"),
         kernels=(b"ledger_batch_kernel",), no_device="no device: no workspace, hence no ledger",
         structs={"row": ("LedgerRow", 192, dict(call=0, n_terms=8, n_reservoirs=12, time=16, potential=24, cavity=56,
                                                 cavity_potential=80, potential_total=88, kinetic_group=96, kinetic_cavity=104,
                                                 kinetic_total=112, system_total=120, reservoir=128, reservoir_total=160,
                                                 universe_total=168, temperature=176, reserved=184)),
                  "item": ("LedgerItem", 128, dict(d_result=0, d_vel=8, d_members=16, n_members=24, N=28, d_energy=32,
                                                   d_reservoir=64, d_time=96, dof=104, add_cavity_kinetic=112, reserved0=116,
                                                   reserved=120))},
         dtypes={"row": "ledger_row_dtype"}, good=abi.good_ledger, without_handle=("item_check",),
         create=lambda capi, it: (1, byref(it), 8, 1, KB),
         with_handle=lambda capi, it: {"set_items": (0, 1, byref(it)), "record": (None,),
                                       "rows": (None, byref(ctypes.c_uint64())),
                                       "read": (None, 0, 1, 0, 1, byref(capi.LedgerRow())), "reset": (None,),
                                       "device_ptr": (byref(vp()), byref(vp()))},
         handle="Ledger", handle_methods=("record", "rows", "read", "reset", "set_items", "device_ptr", "close"),
         cls="BatchEnergyLedger", module="ledger", methods=("record", "rows", "read", "reset", "close"), properties=(),
         on_cpu=_ledger_on_cpu),
    _row("thermalize",
         entry_points=("item_check", "create", "destroy", "set_items", "run", "read", "reset", "state_device_ptr"),
         kernels=(b"thermalize_batch_kernel",), no_device="no device: no workspace, hence no thermalize object",
         structs={"item": ("ThermalizeItem", 160, dict(d_vel=0, d_members=8, d_pos=16, d_image=24, d_result=32, seed=40, kT=48,
                                                       N=56, n_members=60, flags=64, reserved0=68, L=72, params=96, reserved=128)),
                  "state": ("ThermalizeState", 64, dict(draws=0, thermalised=8, skipped=16, momentum=24, photon=48, reserved0=52,
                                                        reserved=56))},
         dtypes={"state": "thermalize_state_dtype"}, good=abi.good_thermalize, without_handle=("item_check",),
         create=lambda capi, it: (1, byref(it)),
         with_handle=lambda capi, it: {"set_items": (0, 1, byref(it)), "run": (None,),
                                       "read": (None, byref(capi.ThermalizeState())), "reset": (None,),
                                       "state_device_ptr": (byref(vp()),)},
         handle="Thermalize", handle_methods=("run", "read", "reset", "set_items", "state_device_ptr", "close"),
         cls="BatchThermalizer", module="thermalize_batch", methods=("thermalize", "state", "reset", "close", "update"),
         properties=("thermalizer",), on_cpu=_thermalize_on_cpu),
    _row("draw",
         entry_points=("item_check", "create", "destroy", "set_items", "fill", "read", "reset", "state_device_ptr"),
         kernels=(b"draw_fill_kernel",), no_device="no device: no workspace, hence no draw object",
         structs={"item": ("DrawItem", 160, dict(d_verlet_row=0, d_bussi_row=8, d_records=16, d_rows=24, capacity=32,
                                                 langevin_gamma=40, bussi_set_T=56, dt_initial=80, tolerance_target=88, dt_min=112,
                                                 dt_max=120, reserved=128)),
                  "state": ("DrawState", 64, dict(draws=0, dt=8, elapsed=16, tolerance=24, exhausted=32, reserved=40))},
         dtypes={"state": "draw_state_dtype"}, good=abi.good_draw, without_handle=("item_check",),
         create=lambda capi, it: (7, 1, byref(it)),
         with_handle=lambda capi, it: {"set_items": (0, 1, byref(it)), "fill": (None,), "read": (None, byref(capi.DrawState())),
                                       "reset": (None,), "state_device_ptr": (byref(vp()),)},
         handle="Draw", handle_methods=("fill", "read", "reset", "set_items", "state_device_ptr", "close"),
         cls="StepDraw", module="step_draw", methods=("fill", "state", "reset", "close"), properties=("draw",),
         on_cpu=_draw_on_cpu),
    _row("molecular",
         entry_points=("pair_make", "params_check", "item_check", "create", "destroy", "set_items", "compute", "order"),
         kernels=(b"molecular_force_kernel",), no_device="no device: no workspace, hence no molecular batch",
         structs={"pair": ("MolecularPair", 64, {}), "bond_params": ("MolecularBondParams", 16, {}),
                  "params": ("MolecularParams", 4240, dict(pair=16, bond=4112)), "bond": ("MolecularBond", 12, {}),
                  "item": ("MolecularItem", 64, dict(N=48))},
         dtypes={}, good=abi.good_molecular, without_handle=("pair_make", "params_check", "item_check", "order"),
         create=lambda capi, it: (byref(abi.molecular_params(capi)), 1, byref(it)),
         with_handle=lambda capi, it: {"set_items": (0, 1, byref(it)), "compute": (None,)},
         handle="Molecular", handle_methods=("compute", "set_items", "close"),
         cls="MolecularForceBatch", module="molecular_batch", methods=("compute", "potential_energy", "close"),
         properties=("forces",), on_cpu=_molecular_on_cpu),
    _row("coulomb",
         entry_points=("item_check", "k_count", "parameters", "order", "create", "destroy", "set_items", "compute",
                       "structure_device_ptr"),
         kernels=(b"coulomb_structure_kernel", b"coulomb_force_kernel"),
         no_device="no device: no workspace, hence no Coulomb batch",
         structs={"item": ("CoulombItem", 96, dict(Lx=32, kappa=56, N=80))},
         dtypes={}, good=abi.good_coulomb, without_handle=("item_check", "k_count", "parameters", "order"),
         create=lambda capi, it: (1, byref(it)),
         with_handle=lambda capi, it: {"set_items": (0, 1, byref(it)), "compute": (None,), "structure_device_ptr": (None, None)},
         handle="Coulomb", handle_methods=("compute", "set_items", "close", "structure_device_ptr"),
         cls="CoulombForceBatch", module="coulomb_batch", methods=("compute", "potential_energy", "close"),
         properties=("forces",), on_cpu=_coulomb_on_cpu),
]
ROWS = {obj.name: obj for obj in OBJECTS}


def _names(obj):
    return {obj.prefix + "_" + s for s in obj.entry_points}


def _applies(obj, check):
    if check in obj.skip:
        pytest.skip(obj.skip[check])


# ---- a. the header ------------------------------------------------------------------------------------------------------
def header_declares_exactly_the_entry_points(obj):
    _applies(obj, "a")
    declared = abi.declared(obj.prefix + "_")
    assert declared == sorted(_names(obj)), set(declared) ^ _names(obj)
    assert "typedef struct %s %s;" % (obj.typedef, obj.typedef) in abi.header_text(), obj.typedef


# ---- b. the libraries ---------------------------------------------------------------------------------------------------
def libraries_export_the_entry_points_and_nothing_stray(obj, capi):
    _applies(obj, "b")
    for path in (capi.LIB_PATH, capi.HOOKS_LIB_PATH):
        lib = ctypes.CDLL(path)
        for name in _names(obj):
            assert hasattr(lib, name), (path, name)
        exported = {s for s in abi.exported(path) if s.startswith(obj.prefix + "_")}
        assert exported == _names(obj), (path, exported ^ _names(obj))
    blob = open(capi.LIB_PATH, "rb").read()
    assert b"gfx950" in blob
    for kernel in obj.kernels:
        assert kernel in blob, kernel


# ---- c. the version -----------------------------------------------------------------------------------------------------
def the_version_is_still_2(capi):
    assert re.search(r"#define\s+CAVMD_VERSION_MINOR\s+2\b", abi.header_text()), "CAVMD_VERSION_MINOR is not 2"
    assert capi.load().cavmd_version() == 2, capi.load().cavmd_version()


# ---- d. the C99 caller and the layouts ----------------------------------------------------------------------------------------
def c99_caller_runs_and_its_layouts_equal_ctypes_and_numpy(obj, capi, tmp_path):
    """tests/c_abi/<object>_abi_check.c prints sizeof and offsetof of every field as the C compiler sees them; they equal the
    ctypes structures field by field, the sizes and offsets pinned in the table, and the numpy dtype where there is one.  The
    program also runs the refusals seen from C.  Returns what the program printed."""
    _applies(obj, "d")
    stdout = abi.run_c99(obj.program, capi, tmp_path)
    assert obj.ok in stdout, stdout
    if not torch.cuda.is_available():
        assert obj.no_device in stdout, stdout
    sizes, offsets = abi.c_layouts(stdout)
    assert sizes == {which: size for which, (_, size, _) in obj.structs.items()}, sizes
    for which, (struct, size, anchors) in obj.structs.items():
        S = getattr(capi, struct)
        in_ctypes = {name: getattr(S, name).offset for name, *_ in S._fields_}
        assert ctypes.sizeof(S) == size, (which, ctypes.sizeof(S))
        assert offsets[which] == in_ctypes, (which, "C", offsets[which], "ctypes", in_ctypes)
        assert {name: offsets[which][name] for name in anchors} == anchors, (which, offsets[which])
    for which, maker in obj.dtypes.items():
        S, dt = getattr(capi, obj.structs[which][0]), getattr(capi, maker)()
        assert dt.itemsize == sizes[which] and set(dt.names) == set(offsets[which]), (which, dt)
        for name in dt.names:
            assert dt.fields[name][1] == offsets[which][name], (which, name, "numpy offset", dt.fields[name][1])
            assert dt.fields[name][0].itemsize == getattr(S, name).size, (which, name, "numpy size", dt.fields[name][0].itemsize)
            ctype = dict((f[0], f[1]) for f in S._fields_)[name]
            shape = (ctype._length_,) if issubclass(ctype, ctypes.Array) else ()
            assert dt.fields[name][0].shape == shape, (which, name, "numpy shape", dt.fields[name][0].shape, "ctypes", shape)
    return stdout


# ---- e. null arguments --------------------------------------------------------------------------------------------------
def null_arguments_are_refused_without_a_device(obj, capi):
    _applies(obj, "e")
    lib = capi.load()
    INV = capi.CAVMD_ERR_INVALID_VALUE
    it = obj.good(capi)
    calls = obj.with_handle(capi, it)
    covered = list(calls) + ["create", "destroy"] + list(obj.without_handle)
    assert sorted(covered) == sorted(obj.entry_points), set(covered) ^ set(obj.entry_points)
    out = vp(123)
    create = getattr(lib, obj.prefix + "_create")
    assert create(None, *obj.create(capi, it), byref(out)) == INV and not out.value, "create without a workspace"
    assert create(None, *obj.create(capi, it), None) == INV, "create without an out pointer"
    assert getattr(lib, obj.destroy)(None) == 0, "destroy(NULL)"
    for name, args in calls.items():
        assert getattr(lib, obj.prefix + "_" + name)(None, *args) == INV, name


# ---- g. the launch order ------------------------------------------------------------------------------------------------
def _size_lists():
    """50 random size lists from each of three seeded generators (seeds 5, 11 and 12), the largest sizes 20001 and 65536"""
    lists = []
    for seed, choices in ((5, [0, 1, 64, 501, 501, 501, 1024, 4096, 20001]), (11, [0, 1, 64, 501, 501, 501, 1024, 4097, 65536]),
                          (12, [0, 1, 64, 501, 501, 501, 1024, 4097, 65536])):
        rng = random.Random(seed)
        lists += [[rng.choice(choices) for _ in range(rng.randrange(1, 200))] for _ in range(50)]
    return lists


SIZE_LISTS = _size_lists()
KNOWN_ORDERS = (([5, 0, 7, 5, 7], [2, 4, 0, 3, 1]), ([501] * 8, list(range(8))), ([501, 0, 2049, 501], [2, 0, 3, 1]))


def launch_order_is_a_stable_descending_sort(obj, capi):
    _applies(obj, "g")
    h = object.__new__(getattr(capi, obj.handle))
    for sizes in SIZE_LISTS:
        want = sorted(range(len(sizes)), key=lambda i: -sizes[i])           # sorted() is stable: ties stay in item order
        h.sizes = sizes
        assert h.launch_order == want and capi.batch_launch_order(sizes) == want, (sizes, h.launch_order)
    for sizes, want in KNOWN_ORDERS:
        h.sizes = sizes
        assert h.launch_order == want and capi.batch_launch_order(sizes) == want, (sizes, h.launch_order)


# ---- h. the Python surface ----------------------------------------------------------------------------------------------
def python_class_is_exported_and_refuses_cpu_tensors(obj, capi):
    _applies(obj, "h")
    import importlib

    import cavitymd
    assert obj.cls in cavitymd.__all__, obj.cls + " is not in cavitymd.__all__"
    cls = getattr(cavitymd, obj.cls)
    assert cls is getattr(importlib.import_module("cavitymd." + obj.module), obj.cls), obj.module
    for name in obj.methods:
        assert callable(getattr(cls, name)), name
    for name in obj.properties:
        assert isinstance(getattr(cls, name), property), name
    for name in obj.handle_methods:
        assert callable(getattr(getattr(capi, obj.handle), name)), name
    calls = obj.on_cpu(cavitymd)
    assert calls, "no constructor call in the row"
    for call in calls:
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            call()


# ---- i. deferred destroy ------------------------------------------------------------------------------------------------
def deferred_destroy_takes_the_object_before_its_workspace(obj, capi, monkeypatch):
    _applies(obj, "i")
    order = []
    lib = SimpleNamespace(cavmd_destroy=lambda h: order.append(("ws", h.value)) or 0)
    setattr(lib, obj.destroy, lambda h: order.append((obj.name, h.value)) or 0)
    assert getattr(capi, obj.handle)._PREFIX + "_destroy" == obj.destroy, getattr(capi, obj.handle)._PREFIX
    ws = object.__new__(capi.Workspace)
    ws._lib, ws._h = lib, vp(0x10)
    b = object.__new__(getattr(capi, obj.handle))
    b._lib, b._h, b._ws = lib, vp(0x20), ws
    monkeypatch.setattr(capi, "_capturing", lambda: True)
    ws.close()
    b.close()
    assert order == [] and not b._h.value and not ws._h.value, order
    monkeypatch.setattr(capi, "_capturing", lambda: False)
    capi._destroy_deferred()
    assert order == [(obj.name, 0x20), ("ws", 0x10)], order
    assert not capi._deferred and not capi._deferred_children, (capi._deferred, capi._deferred_children)
