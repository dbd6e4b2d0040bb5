"""The trajectory object (cavmd_trajectory_*) on a machine WITHOUT a GPU: the shared checks a, b, d, e, g, h and i of
tests/batch_objects.py on a row of this file's own, the order of its ten entry points, the layout function against the header's
formulas, every refusal of its item check, the literal layouts of its three structures, the header's prose, and the numpy
mirror of the call rule and of a frame's bytes (tests/trajectory_mirror.py) against hand-worked cases."""
import ctypes
import math

import numpy as np
import pytest
import torch

import batch_objects as checks
import trajectory_mirror as mirror
from abi_support import HEADER

byref, vp = ctypes.byref, ctypes.c_void_p
SIZES = (1, 2, 3, 4, 5, 255, 256, 257, 501, 65536)


def _good(capi, **kw):
    args = dict(pos_ptr=0x10000, image_ptr=0x20004, vel_ptr=0x30000, time_ptr=0x40008, box_L=(10.0, 11.0, 12.0), N=501)
    args.update(kw)
    return capi.trajectory_item(**args)


def _on_cpu(cavitymd):
    from cavitymd import synthetic
    cfg = synthetic.config1()
    pd = cavitymd.ParticleData.from_arrays(cfg["position"], cfg["typeid"], cfg["charge"], cfg["image"], cfg["types"], cfg["box"],
                                           device="cpu")
    sysdef = cavitymd.SystemDefinition(pd)
    vel = torch.zeros((pd.getN(), 4), dtype=torch.float64)
    return [lambda: cavitymd.BatchTrajectoryRecorder([sysdef], [vel], capacity=4),
            lambda: cavitymd.BatchTrajectoryRecorder([sysdef], None, capacity=4),
            lambda: cavitymd.BatchTrajectoryRecorder([sysdef], [np.zeros((pd.getN(), 4))], capacity=4, dtype="f64")]


ROW = checks._row(
    "trajectory",
    entry_points=("item_check", "layout", "create", "destroy", "set_items", "record", "rows", "read", "reset", "device_ptr"),
    kernels=(b"trajectory_batch_kernelILi256ELi0E", b"trajectory_batch_kernelILi256ELi1E"),
    no_device="no device: no workspace, hence no trajectory object",
    structs={"item": ("TrajectoryItem", 64, dict(d_pos=0, d_image=8, d_vel=16, d_time=24, Lx=32, Ly=40, Lz=48, N=56, reserved0=60)),
             "header": ("TrajectoryHeader", 64, dict(call=0, row=8, time=16, N=24, flags=28, box=32, reserved=56)),
             "layout": ("TrajectoryLayout", 48, dict(frame_bytes=0, position_offset=8, velocity_offset=16, image_offset=24, max_N=32,
                                                     format=36, element_bytes=40, reserved=44))},
    dtypes={"header": "trajectory_header_dtype"}, good=_good, without_handle=("item_check", "layout"),
    create=lambda capi, it: (1, byref(it), 501, 1, 8, 1, 0.0),
    with_handle=lambda capi, it: {"set_items": (0, 1, byref(it)), "record": (None, None),
                                  "rows": (None, byref(ctypes.c_uint64())), "read": (None, 0, 1, 0, 1, byref(ctypes.c_uint64())),
                                  "reset": (None,), "device_ptr": (byref(vp()), byref(vp()))},
    handle="Trajectory", handle_methods=("record", "rows", "read", "reset", "set_items", "device_ptr", "close"),
    cls="BatchTrajectoryRecorder", module="trajectory",
    methods=("record", "rows", "read", "unwrapped", "gsd_chunks", "save_npz", "reset", "restore", "close"), properties=(),
    on_cpu=_on_cpu)
ITEM_FIELDS, HEADER_FIELDS, LAYOUT_FIELDS = (ROW.structs[k][2] for k in ("item", "header", "layout"))


# ---- the checks every batch object gets (tests/batch_objects.py), on this file's row -----------------------------------------
def test_header_declares_the_ten_entry_points_and_the_contract():
    checks.header_declares_exactly_the_entry_points(ROW)                                                    # a
    text = " ".join(open(HEADER).read().replace("*", " ").split())
    for words in ("calls += 1; forced = d_take_frame != NULL && d_take_frame[item] != 0", "phase += 1; due = phase >= period",
                  "t = d_time; due = rows == 0 || t - last_time >= time_interval", "a NaN time is never due",
                  "the frame goes to slot rows % capacity", "last_time = d_time (or 0) and phase = 0", "rows += 1",
                  "src/cavitymd/analysis.py:366-378", "write_at_start", "examples/05_advanced_run.py:1231-1246",
                  "round to nearest even", "are written as zero"):
        assert words in text, words
    raw = open(HEADER).read()
    assert raw.index("cavmd_coulomb_structure_device_ptr(") < raw.index("typedef struct cavmd_trajectory_item") \
        < raw.index("cavmd_trajectory_device_ptr(") < raw.index("measurement hooks")
    assert "hoomd.write.GSD" in raw[:raw.index("#ifndef CAVMD_H_")]           # the reference-interface table
    assert "#define CAVMD_TRAJECTORY_F64 0" in raw and "#define CAVMD_TRAJECTORY_F32 1" in raw


def test_libraries_export_them_and_prototypes_follow_the_headers_order(capi):
    checks.libraries_export_the_entry_points_and_nothing_stray(ROW, capi)                                   # b
    names = [n for n in capi._PROTOTYPES if n.startswith("cavmd_trajectory_")]
    assert names == ["cavmd_trajectory_" + s for s in ROW.entry_points]
    raw = open(HEADER).read()
    at = [raw.index("CAVMD_API int %s(" % n) for n in names]
    assert at == sorted(at)                                                  # header and _PROTOTYPES: one order
    order = list(capi._PROTOTYPES)
    assert order.index("cavmd_coulomb_structure_device_ptr") + 1 == order.index("cavmd_trajectory_item_check")
    assert order.index("cavmd_trajectory_device_ptr") + 1 == order.index("cavmd_profile_enable")


def test_c_layouts_equal_the_ctypes_ones_and_the_numpy_dtype(capi, tmp_path):
    checks.c99_caller_runs_and_its_layouts_equal_ctypes_and_numpy(ROW, capi, tmp_path)                      # d
    for S, fields, size in ((capi.TrajectoryItem, ITEM_FIELDS, 64), (capi.TrajectoryHeader, HEADER_FIELDS, 64),
                            (capi.TrajectoryLayout, LAYOUT_FIELDS, 48)):
        assert ctypes.sizeof(S) == size and {name: getattr(S, name).offset for name, *_ in S._fields_} == fields
    dt = capi.trajectory_header_dtype()
    assert dt.itemsize == 64 and {n: dt.fields[n][1] for n in dt.names} == HEADER_FIELDS
    assert {n: mirror.HEADER_DTYPE.fields[n][1] for n in mirror.HEADER_DTYPE.names} == HEADER_FIELDS
    # the dtype of a whole frame: the header's columns and the three sections at the layout's offsets
    for fmt, element in ((capi.TRAJECTORY_F64, "<f8"), (capi.TRAJECTORY_F32, "<f4")):
        lay = capi.trajectory_layout(501, fmt)
        frame = capi.trajectory_frame_dtype(lay)
        assert frame.itemsize == lay.frame_bytes and frame.names[:7] == dt.names
        assert [frame.fields[n][1] for n in ("position", "velocity", "image")] == [lay.position_offset, lay.velocity_offset,
                                                                                  lay.image_offset]
        assert frame.fields["position"][0] == np.dtype((element, (501, 3))) == frame.fields["velocity"][0]
        assert frame.fields["image"][0] == np.dtype(("<i4", (501, 3)))


def test_null_arguments_are_refused_without_a_device(capi):
    checks.null_arguments_are_refused_without_a_device(ROW, capi)                                           # e
    lib = capi.load()
    assert lib.cavmd_trajectory_record(None, None, vp(0x1002)) == capi.CAVMD_ERR_INVALID_VALUE


def test_launch_order_is_a_stable_descending_sort(capi):
    checks.launch_order_is_a_stable_descending_sort(ROW, capi)                                              # g
    assert capi.Trajectory._size(_good(capi, N=77)) == 77


def test_python_class_is_exported_and_refuses_cpu_tensors(capi):
    checks.python_class_is_exported_and_refuses_cpu_tensors(ROW, capi)                                      # h
    import cavitymd
    doc = cavitymd.trajectory.__doc__
    step = doc[doc.index("with torch.cuda.graph(graph):"):]
    order = [step.index(call) for call in ("draw.fill()", "integrator.step_one()", "integrator.step_two()", "trajectory.record()")]
    assert order == sorted(order)


def test_deferred_destroy_takes_the_object_before_its_workspace(capi, monkeypatch):
    checks.deferred_destroy_takes_the_object_before_its_workspace(ROW, capi, monkeypatch)                   # i


# ---- the layout function ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt", (0, 1))
def test_layout_follows_the_formulas(capi, fmt):
    e = 8 if fmt == 0 else 4
    pad16 = lambda x: -(-x // 16) * 16
    for n in SIZES:
        lay = capi.trajectory_layout(n, fmt)
        got = {name: int(getattr(lay, name)) for name, _ in capi.TrajectoryLayout._fields_}
        velocity = 64 + pad16(3 * n * e)
        image = velocity + pad16(3 * n * e)
        want = dict(frame_bytes=image + pad16(12 * n), position_offset=64, velocity_offset=velocity, image_offset=image, max_N=n,
                    format=fmt, element_bytes=e, reserved=0)
        assert got == want == mirror.layout(n, fmt), (n, got, want)
        assert all(got[k] % 16 == 0 for k in ("frame_bytes", "position_offset", "velocity_offset", "image_offset"))


def test_layout_refusals(capi):
    lib, INV = capi.load(), capi.CAVMD_ERR_INVALID_VALUE
    out = capi.TrajectoryLayout()
    M = capi.BATCH_MAX_ITEM_N
    assert lib.cavmd_trajectory_layout(M, 0, byref(out)) == 0 and lib.cavmd_trajectory_layout(1, 1, byref(out)) == 0
    for n, fmt in ((0, 0), (0, 1), (M + 1, 0), (M + 1, 1), (2 ** 32 - 1, 0), (501, 2), (501, 3), (501, 2 ** 32 - 1)):
        assert lib.cavmd_trajectory_layout(n, fmt, byref(out)) == INV, (n, fmt)
    assert lib.cavmd_trajectory_layout(501, 0, None) == INV
    with pytest.raises(capi.CavmdError):
        capi.trajectory_layout(0, 0)
    assert capi.TRAJECTORY_MAX_BYTES == 2 ** 32 and (capi.TRAJECTORY_F64, capi.TRAJECTORY_F32) == (0, 1)


# ---- refusals of the item check ---------------------------------------------------------------------------------------------
def test_item_check_refusals(capi):
    lib = capi.load()
    INV, CAP = capi.CAVMD_ERR_INVALID_VALUE, capi.CAVMD_ERR_CAPACITY
    chk = capi.trajectory_item_check
    assert lib.cavmd_trajectory_item_check(None) == INV
    assert chk(_good(capi)) == 0
    assert chk(capi.TrajectoryItem()) == 0                                   # N == 0: nothing is required
    assert chk(_good(capi, vel_ptr=0)) == 0 and chk(_good(capi, time_ptr=0)) == 0 and chk(_good(capi, vel_ptr=0, time_ptr=0)) == 0
    # alignments: 16 for d_pos and d_vel, 4 for d_image, 8 for d_time -- with N == 0 as well
    for N in (501, 0):
        for off in (1, 2, 4, 8):
            assert chk(_good(capi, N=N, pos_ptr=0x10000 + off)) == INV, (N, off)
            assert chk(_good(capi, N=N, vel_ptr=0x30000 + off)) == INV, (N, off)
        for off, status in ((1, INV), (2, INV), (3, INV), (4, 0), (8, 0), (12, 0)):
            assert chk(_good(capi, N=N, image_ptr=0x20000 + off)) == status, (N, off)
        for off, status in ((1, INV), (2, INV), (4, INV), (8, 0), (16, 0)):
            assert chk(_good(capi, N=N, time_ptr=0x40000 + off)) == status, (N, off)
    # d_pos and d_image are required with N > 0 only
    assert chk(_good(capi, pos_ptr=0)) == INV and chk(_good(capi, image_ptr=0)) == INV
    assert chk(_good(capi, N=1, pos_ptr=0)) == INV and chk(_good(capi, N=1, image_ptr=0)) == INV
    assert chk(_good(capi, N=0, pos_ptr=0, image_ptr=0)) == 0
    # the box: finite and > 0 with N > 0; not looked at with N == 0
    for bad in (0.0, -0.0, -1.0, float("nan"), float("inf"), float("-inf")):
        for axis in range(3):
            box = [10.0, 11.0, 12.0]
            box[axis] = bad
            assert chk(_good(capi, box_L=box)) == INV, (axis, bad)
            assert chk(_good(capi, box_L=box, N=0)) == 0, (axis, bad)
    assert chk(_good(capi, box_L=(5e-324, 1e308, 1.0))) == 0
    # the cap
    M = capi.BATCH_MAX_ITEM_N
    assert chk(_good(capi, N=M)) == 0 and chk(_good(capi, N=M + 1)) == CAP and chk(_good(capi, N=2 ** 32 - 1)) == CAP
    # the reserved word
    for value in (1, 2 ** 31, 2 ** 32 - 1):
        for N in (501, 0):
            it = _good(capi, N=N)
            it.reserved0 = value
            assert chk(it) == INV, (value, N)
    # precedence, as the ledger's: the reserved word, pointers and values before the capacity
    it = _good(capi, N=M + 1)
    it.reserved0 = 1
    assert chk(it) == INV
    assert chk(_good(capi, N=M + 1, vel_ptr=0x30008)) == INV and chk(_good(capi, N=M + 1, pos_ptr=0)) == INV
    assert chk(_good(capi, N=M + 1, box_L=(1.0, 0.0, 1.0))) == INV


# ---- the mirror against hand-worked cases -------------------------------------------------------------------------------------
def _run(period, interval, calls, capacity=100):
    """calls: (time, forced) per call; returns the (call, row, forced) of every frame and the item"""
    it, frames = mirror.Item(), []
    for time, forced in calls:
        head = it.call(capacity, period, interval, time, forced)
        if head is not None:
            frames.append((head["call"], head["row"], head["forced"]))
    return frames, it


def test_mirror_step_rule_period_3():
    frames, it = _run(3, 0.0, [(None, False)] * 10)
    assert frames == [(3, 0, False), (6, 1, False), (9, 2, False)]
    assert (it.rows, it.calls, it.phase, it.slot, it.last_time) == (3, 10, 1, 3, 0.0)
    # a forced frame on call 4 restarts the phase: the next due call is 7, not 6
    frames, it = _run(3, 0.0, [(None, k == 3) for k in range(10)])
    assert frames == [(3, 0, False), (4, 1, True), (7, 2, False), (10, 3, False)]
    assert (it.rows, it.calls, it.phase) == (4, 10, 0)
    # a forced frame on a due call is forced and due: one frame, flagged
    frames, _ = _run(3, 0.0, [(None, k == 2) for k in range(3)])
    assert frames == [(3, 0, True)]
    # period 1: every call
    assert _run(1, 0.0, [(None, False)] * 3)[0] == [(1, 0, False), (2, 1, False), (3, 2, False)]


def test_mirror_time_rule_equality_one_ulp_below_and_nan():
    T = 0.3
    # the first call records whatever the clock says; then t - last >= T by ONE subtraction and ONE comparison
    exact = 1.0 + T                               # 1.3: 1.3 - 1.0 rounds to 0.30000000000000004 >= 0.3
    assert exact - 1.0 >= T
    frames, it = _run(1, T, [(1.0, False), (1.2, False), (exact, False)])
    assert frames == [(1, 0, False), (3, 1, False)] and it.last_time == exact and it.phase == 0
    # t - last exactly equal to the interval: due.  0.5 and 0.25 are exact in binary.
    frames, _ = _run(1, 0.25, [(0.5, False), (0.75, False)])
    assert frames == [(1, 0, False), (2, 1, False)]
    # one ulp below: not due; the next representable time is
    below = math.nextafter(0.75, 0.0)
    assert below - 0.5 < 0.25
    frames, it = _run(1, 0.25, [(0.5, False), (below, False), (0.75, False)])
    assert frames == [(1, 0, False), (3, 1, False)] and it.calls == 3
    # a NaN time is never due by the comparison; the clock coming back is
    frames, it = _run(1, 0.25, [(0.0, False), (float("nan"), False), (float("nan"), False), (0.25, False)])
    assert frames == [(1, 0, False), (4, 1, False)] and it.last_time == 0.25
    # a NaN time that is forced records and moves last_time to NaN: nothing is due after it until a forced frame or a reset
    frames, it = _run(1, 0.25, [(0.0, False), (float("nan"), True), (100.0, False), (200.0, True), (200.25, False)])
    assert frames == [(1, 0, False), (2, 1, True), (4, 2, True), (5, 3, False)]
    # an infinite time: inf - last >= T once, then inf - inf is NaN
    frames, _ = _run(1, 0.25, [(0.0, False), (float("inf"), False), (float("inf"), False)])
    assert frames == [(1, 0, False), (2, 1, False)]


def test_mirror_forced_frame_moves_last_time_and_reset_records_again():
    # frames at 0 and (forced) 0.2; 0.3 is then only 0.1 after the last frame; 0.5 is due
    frames, it = _run(1, 0.25, [(0.0, False), (0.2, True), (0.3, False), (0.5, False)])
    assert frames == [(1, 0, False), (2, 1, True), (4, 2, False)] and it.last_time == 0.5
    it.reset()
    assert (it.rows, it.calls, it.phase, it.slot, it.last_time) == (0, 0, 0, 0, 0.0)
    assert it.call(100, 1, 0.25, 0.5, False) == dict(call=1, row=0, time=0.5, forced=False, slot=0)   # rows == 0: at once
    # the ring: the slot is rows % capacity
    it = mirror.Item()
    slots = [it.call(4, 1, 0.0, None, False)["slot"] for _ in range(11)]
    assert slots == [0, 1, 2, 3, 0, 1, 2, 3, 0, 1, 2] and it.slot == 3 and it.rows == 11


@pytest.mark.parametrize("fmt", (0, 1))
def test_mirror_frame_bytes_hand_worked(fmt):
    """max_N = 3, N = 1: which bytes a frame writes, which it leaves, and the F32 conversion at its edges"""
    lay = mirror.layout(3, fmt)
    e = lay["element_bytes"]
    assert lay == dict(frame_bytes={8: 64 + 80 + 80 + 48, 4: 64 + 48 + 48 + 48}[e], position_offset=64,
                       velocity_offset={8: 144, 4: 112}[e], image_offset={8: 224, 4: 160}[e], max_N=3, format=fmt,
                       element_bytes=e, reserved=0)
    old = np.full(lay["frame_bytes"], 0xAB, dtype=np.uint8)
    tag = np.array([0x7FF0DEADBEEF0001], dtype=np.uint64).view(np.float64)[0]
    pos = np.array([[1.5, -0.0, 1e-40, tag]])
    vel = np.array([[1e39, 2.0 ** -150, float("nan"), tag]])
    image = np.array([[-2 ** 31, 2 ** 31 - 1, 7]], dtype=np.int64)
    head = dict(call=5, row=2, time=0.75, forced=True)
    out = mirror.frame_bytes(lay, old, head, (10.0, 11.0, 12.0), pos, vel, image)
    h = out[:64].view(mirror.HEADER_DTYPE)[0]
    assert (h["call"], h["row"], h["time"], h["N"], h["flags"], h["reserved"]) == (5, 2, 0.75, 1, 3, 0)
    assert h["box"].tolist() == [10.0, 11.0, 12.0]
    written = 3 * e                                 # one particle's components; padded with zeros to 16 (F32) or 32 (F64)
    padded = mirror.pad16(written)
    for off in (lay["position_offset"], lay["velocity_offset"]):
        assert not out[off + written:off + padded].any()
        assert (out[off + padded:off + mirror.pad16(9 * e)] == 0xAB).all()          # the rest of the section: as it was
    assert not out[lay["image_offset"] + 12:lay["image_offset"] + 16].any()
    assert (out[lay["image_offset"] + 16:] == 0xAB).all()
    assert out[lay["image_offset"]:lay["image_offset"] + 12].view("<i4").tolist() == [-2 ** 31, 2 ** 31 - 1, 7]
    p = out[lay["position_offset"]:lay["position_offset"] + written]
    v = out[lay["velocity_offset"]:lay["velocity_offset"] + written]
    if fmt == mirror.F64:
        assert p.view("<u8").tolist() == pos[0, :3].view(np.uint64).tolist()
        assert v.view("<u8").tolist() == vel[0, :3].view(np.uint64).tolist()
    else:
        # 1.5; -0.0 keeps its sign; 1e-40 is the subnormal 71362 * 2^-149 (1e-40 / 2^-149 = 71362.38...)
        assert p.view("<u4").tolist() == [0x3FC00000, 0x80000000, 71362]
        # 1e39 is beyond the float range: +inf; 2^-150 is a tie between 0 and 2^-149 and goes to the even one, 0; NaN stays NaN
        assert v.view("<u4").tolist()[:2] == [0x7F800000, 0] and np.isnan(v.view("<f4")[2])
    assert bytes(tag.tobytes()) not in out.tobytes()                          # .w is never copied
    # no velocities: the section is +0 and bit 1 is clear; N == 0: the header alone
    out = mirror.frame_bytes(lay, old, dict(head, forced=False), (10.0, 11.0, 12.0), pos, None, image)
    assert out[:64].view(mirror.HEADER_DTYPE)[0]["flags"] == 0
    assert not out[lay["velocity_offset"]:lay["velocity_offset"] + padded].any()
    out = mirror.frame_bytes(lay, old, head, (0.0, 0.0, 0.0), None, None, None)
    assert out[:64].view(mirror.HEADER_DTYPE)[0]["N"] == 0 and (out[64:] == 0xAB).all()
