"""Every no-GPU check of tests/batch_objects.py on every row of its table: the eleven batch objects of include/cavmd.h by the
checks a to i.  What is specific to one object (refusal matrices, row makers, mirrors, header prose) is in its own
tests/test_*_abi.py."""
import pytest
import torch

import abi_support as abi
import batch_objects as checks
from batch_objects import OBJECTS

per_object = pytest.mark.parametrize("obj", OBJECTS, ids=[obj.name for obj in OBJECTS])


def test_the_table_has_the_eleven_objects(capi):
    names = ["batch", "bussi_batch", "recorder", "field_recorder", "verlet", "bath", "ledger", "thermalize", "draw", "molecular",
             "coulomb"]
    assert [obj.name for obj in OBJECTS] == names
    assert [len(obj.entry_points) for obj in OBJECTS] == [10, 10, 9, 10, 11, 8, 9, 8, 8, 8, 9]
    handles = {getattr(capi, obj.handle) for obj in OBJECTS}
    assert len(handles) == 11 and all(issubclass(h, capi._ItemTableHandle) for h in handles)
    # the header's order, as _capi._PROTOTYPES has it
    first = [list(capi._PROTOTYPES).index(obj.prefix + "_create") for obj in OBJECTS]
    assert first == sorted(first), first


def test_no_prefix_is_a_prefix_of_another():
    """an entry point belongs to one object: cavmd_bath_ against cavmd_batch_, cavmd_recorder_ against cavmd_field_recorder_"""
    for a in OBJECTS:
        for b in OBJECTS:
            assert a is b or not (a.prefix + "_").startswith(b.prefix + "_"), (a.prefix, b.prefix)


# ---- a. the header ------------------------------------------------------------------------------------------------------
@per_object
def test_header_declares_exactly_the_entry_points(obj):
    checks.header_declares_exactly_the_entry_points(obj)


# ---- b. the libraries ---------------------------------------------------------------------------------------------------
@per_object
def test_libraries_export_the_entry_points_and_nothing_stray(obj, capi):
    checks.libraries_export_the_entry_points_and_nothing_stray(obj, capi)


def test_libraries_export_exactly_what_python_binds(capi):
    """b for all objects at once: with the rows' own names checked above, nothing else leaves either library"""
    for path in (capi.LIB_PATH, capi.HOOKS_LIB_PATH):
        exported = abi.exported(path)
        assert not {s for s in exported if not s.startswith("cavmd_") and not s.startswith("_")}, path
        assert {s for s in exported if s.startswith("cavmd_")} == set(capi.EXPORTED_SYMBOLS), path


# ---- c. the version -----------------------------------------------------------------------------------------------------
def test_the_version_is_still_2(capi):
    checks.the_version_is_still_2(capi)


# ---- d. the C99 caller and the layouts ----------------------------------------------------------------------------------------
@per_object
def test_c99_caller_runs_and_its_layouts_equal_ctypes_and_numpy(obj, capi, tmp_path):
    checks.c99_caller_runs_and_its_layouts_equal_ctypes_and_numpy(obj, capi, tmp_path)


# ---- e. null arguments --------------------------------------------------------------------------------------------------
@per_object
def test_null_arguments_are_refused_without_a_device(obj, capi):
    checks.null_arguments_are_refused_without_a_device(obj, capi)


# ---- f. no device -------------------------------------------------------------------------------------------------------
@pytest.mark.skipif(torch.cuda.is_available(), reason="checks the no-GPU behaviour")
def test_no_device_no_workspace_hence_no_object(capi):
    with pytest.raises(capi.CavmdError) as e:
        capi.Workspace(1)
    assert e.value.status == capi.CAVMD_ERR_NO_DEVICE


# ---- g. the launch order ------------------------------------------------------------------------------------------------
@per_object
def test_launch_order_is_a_stable_descending_sort(obj, capi):
    checks.launch_order_is_a_stable_descending_sort(obj, capi)


# ---- h. the Python surface ----------------------------------------------------------------------------------------------
@per_object
def test_python_class_is_exported_and_refuses_cpu_tensors(obj, capi):
    checks.python_class_is_exported_and_refuses_cpu_tensors(obj, capi)


# ---- i. deferred destroy ------------------------------------------------------------------------------------------------
@per_object
def test_deferred_destroy_takes_the_object_before_its_workspace(obj, capi, monkeypatch):
    checks.deferred_destroy_takes_the_object_before_its_workspace(obj, capi, monkeypatch)
