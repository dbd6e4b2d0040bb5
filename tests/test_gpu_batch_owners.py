"""What the seven user-facing batch classes share above the library: the life of a handle with its workspace, the step's input
rows, and the wait of a replacement for the launches in flight.  B = 3 systems of N = 0, 1 and 5 particles in a box of 20 bohr
(the Coulomb cut-off is 8), one bond / exclusion in the largest."""
import gc
import sys

import numpy as np
import pytest
import torch

import cavitymd
from cavitymd import _capi
from gpu_support import same as _same
from water_systems import HARMONIC, LJ

pytestmark = pytest.mark.gpu

SIZES = (0, 1, 5)
BOX = (20.0, 20.0, 20.0)
R_CUT = 8.0
BONDS = [None, None, [[0, 1]]]
BOND_TYPES = [None, None, [0]]
PARAMS = {"omegac": 0.0091, "couplstr": 1e-3, "phmass": 1.0}
LJ_SHORT = {pair: dict(p, r_cut=R_CUT) for pair, p in LJ.items()}


def _sysdef(n, seed):
    """n particles of types O, N with charges that sum to zero where n > 1; the last one is the photon 'L' where n > 1"""
    rng = np.random.default_rng(seed)
    position = rng.uniform(-0.5, 0.5, (n, 3)) * np.array(BOX)
    if n > 1:
        position[1] = position[0] + (2.3, 0.0, 0.0)                   # the bonded pair, inside the box after the wrap below
        position[1] -= np.array(BOX) * np.round(position[1] / np.array(BOX))
    typeid = np.array([k % 2 for k in range(n)], dtype=np.int32)
    charge = np.array([0.4 * (-1) ** k for k in range(n)], dtype=np.float64)
    if n > 1:
        typeid[-1], charge[-1] = 2, 0.0
    pd = cavitymd.ParticleData.from_arrays(position, typeid, charge, np.zeros((n, 3), dtype=np.int32), ["O", "N", "L"], BOX,
                                           device="cuda")
    return cavitymd.SystemDefinition(pd)


def _sysdefs(seed=0):
    return [_sysdef(n, seed + k) for k, n in enumerate(SIZES)]


def _velocities(seed=3):
    rng = np.random.default_rng(seed)
    return [torch.from_numpy(np.concatenate([rng.normal(size=(n, 3)) * 1e-4, np.full((n, 1), 2.5e4)], axis=1)).cuda() for n in SIZES]


def _cavity(sysdefs):
    return cavitymd.CavityForceBatch(sysdefs, PARAMS)


def _molecular(sysdefs):
    return cavitymd.MolecularForceBatch(sysdefs, BONDS, BOND_TYPES, HARMONIC, LJ_SHORT)


def _coulomb(sysdefs):
    return cavitymd.CoulombForceBatch(sysdefs, BONDS, r_cut=R_CUT, accuracy=1e-4)


def _thermostat(velocities):
    t = cavitymd.BussiReservoirBatch(kT=3.167e-4, tau=0.5)
    t.attach(velocities, translational_dof=[3.0 * n for n in SIZES])
    return t


# ---- 1. life cycle ------------------------------------------------------------------------------------------------------------------
def _owners():
    """(what to keep alive, [(object, its release, a launch of it)]) for all seven classes"""
    sysdefs, velocities = _sysdefs(), _velocities()
    cavity = _cavity(sysdefs)
    thermostat = _thermostat(velocities)
    recorder = cavitymd.BatchRecorder(cavity, velocities, net_forces=cavity.forces, capacity=4)
    fields = cavitymd.BatchFieldRecorder([s.getParticleData().getPositions() for s in sysdefs], num_wavevectors=3, capacity=4,
                                         max_references=2)
    verlet = cavitymd.VerletBatch(cavity, velocities)
    molecular, coulomb = _molecular(sysdefs), _coulomb(sysdefs)
    # the objects built over the cavity batch's arrays go before it
    return (sysdefs, velocities), [(recorder, recorder.close, recorder.record), (fields, fields.close, fields.record),
                                   (verlet, verlet.close, verlet.step_one), (thermostat, thermostat.detach, thermostat.step_async),
                                   (molecular, molecular.close, molecular.compute), (coulomb, coulomb.close, coulomb.compute),
                                   (cavity, cavity.close, cavity.compute)]


def test_release_twice_is_quiet_and_a_launch_afterwards_names_the_class():
    keep, owners = _owners()
    for obj, release, launch in owners:
        launch()
    torch.cuda.synchronize()
    for obj, release, launch in owners:
        release()
        release()
        assert obj._ws is None and obj.workspace is None
        with pytest.raises(RuntimeError, match=type(obj).__name__):
            launch()


def test_dropping_the_last_reference_without_closing_is_quiet():
    raised = []
    hook, sys.unraisablehook = sys.unraisablehook, raised.append
    try:
        keep, owners = _owners()
        for obj, release, launch in owners:
            launch()
        torch.cuda.synchronize()
        workspaces = [obj._ws for obj, _, _ in owners]
        while owners:                                                 # in order: the cavity batch goes last
            del owners[0]
            obj = release = launch = None
            gc.collect()
    finally:
        sys.unraisablehook = hook
    assert not raised, [str(u.exc_value) for u in raised]
    assert all(not ws.handle.value for ws in workspaces)              # every workspace was destroyed with its owner


@pytest.mark.parametrize("which", ["recorder", "field_recorder"])
def test_a_refused_constructor_leaves_no_workspace_behind(which):
    sysdefs, velocities = _sysdefs(), _velocities()
    cavity = _cavity(sysdefs)
    positions = [s.getParticleData().getPositions() for s in sysdefs]

    def construct(obj, bad):
        if which == "recorder":
            obj.__init__(cavity, velocities, capacity=0 if bad else 4)
        else:
            obj.__init__(positions, num_wavevectors=3, capacity=4, max_references=0 if bad else 2)

    cls = cavitymd.BatchRecorder if which == "recorder" else cavitymd.BatchFieldRecorder
    obj = cls.__new__(cls)
    with pytest.raises(_capi.CavmdError) as e:
        construct(obj, bad=True)
    assert e.value.status == _capi.CAVMD_ERR_INVALID_VALUE
    assert obj._ws is None and obj.recorder is None
    obj.close()                                                       # and releasing what was never opened is quiet
    good = cls.__new__(cls)
    construct(good, bad=False)
    good.record()
    torch.cuda.synchronize()
    assert good.rows().tolist() == [1, 1, 1]
    good.close()
    cavity.close()


# ---- 2. the step's input rows ---------------------------------------------------------------------------------------------------------
def _stepper(which):
    """(object, set_inputs(variates), columns the variates land in, draw_inputs(dt), what keeps it alive)"""
    velocities = _velocities()
    if which == "thermostat":
        t = _thermostat(velocities)
        return t, (lambda v: t.set_inputs(0, 0.5, v)), slice(0, 2), (lambda dt: t.draw_inputs(0, dt)), velocities
    sysdefs = _sysdefs()
    cavity = _cavity(sysdefs)
    v = cavitymd.VerletBatch(cavity, velocities, langevin_index=[None, 0, 4])
    return v, (lambda u: v.set_inputs(0.5, 1e-3, 3.167e-4, u)), slice(3, 6), (lambda dt: v.draw_inputs(dt, 1e-3, 3.167e-4)), \
        (cavity, sysdefs, velocities)


@pytest.mark.parametrize("which", ["thermostat", "integrator"])
def test_step_inputs_keep_their_address_their_last_rows_and_their_constants(which):
    obj, set_inputs, columns, draw_inputs, keep = _stepper(which)
    width = columns.stop - columns.start
    address = obj.inputs.data_ptr()
    assert obj.inputs.shape == (3, 8) and obj.inputs.dtype == torch.float64 and obj.inputs.device.type == "cuda"
    rng = np.random.default_rng(11)
    first, second = rng.uniform(0.1, 0.9, (3, width)), rng.uniform(0.1, 0.9, (3, width))
    set_inputs(first)
    set_inputs(second)                                                # waits for the first copy to have left the staging buffer
    torch.cuda.synchronize()
    assert _same(obj.inputs[:, columns].cpu().numpy(), second)
    assert obj.inputs.data_ptr() == address
    draw_inputs(0.5)
    constants = obj._step_inputs._const
    assert constants is not None
    draw_inputs(0.5)
    assert obj._step_inputs._const is constants                       # the same bytes: not uploaded again
    draw_inputs(0.25)
    assert obj._step_inputs._const is not constants
    torch.cuda.synchronize()
    assert obj.inputs.data_ptr() == address
    assert not _same(obj.inputs[:, columns].cpu().numpy(), second)    # the drawn variates are there
    (obj.detach if which == "thermostat" else obj.close)()


# ---- 3. a replacement waits for the launches in flight -----------------------------------------------------------------------------------
def _replace(which, obj, sysdefs, k):
    """re-registers system k of ``obj`` from sysdefs[k], as the class offers it"""
    pd = sysdefs[k].getParticleData()
    n = pd.getN()
    if which == "cavity":
        obj._sysdefs[k] = sysdefs[k]
        obj.refresh([k])
    elif which == "molecular":
        triples = np.array([[a, b, t] for (a, b), t in zip(BONDS[k] or [], BOND_TYPES[k] or [])], dtype=np.uint32).reshape(-1, 3)
        obj.molecular.set_items(k, [_capi.molecular_item(n, pd.getPositions().data_ptr(), obj.forces[k].data_ptr(), BOX, triples)])
    else:
        obj.coulomb.set_items(k, [_capi.coulomb_item(n, pd.getPositions().data_ptr(), pd.getCharges().data_ptr(),
                                                     obj.forces[k].data_ptr(), BOX, obj.kappa, obj.r_cut, obj.k_cut, BONDS[k])])


@pytest.mark.parametrize("which", ["cavity", "molecular", "coulomb"])
def test_a_replacement_right_after_a_launch_on_a_side_stream_gives_a_fresh_objects_bits(which):
    build = {"cavity": _cavity, "molecular": _molecular, "coulomb": _coulomb}[which]
    k = 2
    sysdefs = _sysdefs()
    moved = list(sysdefs)
    moved[k] = _sysdef(SIZES[k], seed=40)                             # the same system somewhere else, in arrays of its own
    fresh = build(moved)
    fresh.compute()
    torch.cuda.synchronize()
    want = fresh.forces[k].cpu().numpy().copy()
    assert np.isfinite(want).all() and want[:, :3].any()
    obj = build(sysdefs)
    side = torch.cuda.Stream()
    torch.cuda.synchronize()
    obj.compute(stream=side)
    _replace(which, obj, moved, k)                                    # no synchronise in between: the replacement itself waits
    obj.compute(stream=side)
    side.synchronize()
    got = obj.forces[k].cpu().numpy()
    assert _same(got, want)
    for j in (0, 1):                                                  # the neighbours are what they were
        assert _same(obj.forces[j].cpu().numpy(), fresh.forces[j].cpu().numpy())
    obj.close()
    fresh.close()
