"""The shared cavity (cavmd_shared_cavity_*) on a machine WITHOUT a GPU: the header declares exactly its names and states its
contract, a C99 program sees the item's layout and the table rules, every library exports the names and _capi binds them, the two
kernels are in the product's code object, null handles are refused, every rule of cavmd_shared_cavity_table_check on host
tables, and the Python class refuses CPU tensors.  What needs a live object is tests/test_gpu_shared_cavity.py's."""
import ctypes
import re

import pytest

import abi_support as abi

PREFIX = "cavmd_shared_cavity_"
ENTRY_POINTS = ("item_check", "table_check", "create", "destroy", "set_items", "compute", "last_sequence", "results_read",
                "results_device_ptr", "cell_dipoles_device_ptr", "count", "carrier")
NAMES = {PREFIX + s for s in ENTRY_POINTS}
OFFSETS = dict(d_pos=0, d_charge=8, d_image=16, d_force=24, Lx=32, Ly=40, Lz=48, params=56, N=88, L_typeid=92, cavity=96,
               reserved0=100, reserved=104)


def test_header_declares_exactly_the_names_and_states_the_contract():
    assert abi.declared(PREFIX) == sorted(NAMES)
    text = abi.header_text()
    assert "typedef struct cavmd_shared_cavity cavmd_shared_cavity;" in text
    assert re.search(r"#define\s+CAVMD_SHARED_CAVITY_MAX_MEMBERS\s+1024\b", text)
    assert text.index("cavmd_batch_results_device_ptr(") < text.index(PREFIX + "item_check(") < text.index("cavmd_set_wavevectors(")
    assert not [n for n in abi.declared("cavmd_snapshot_") if "shared" in n]          # no device state that a launch advances
    raw = " ".join(open(abi.HEADER).read().replace("*", " ").split())
    for words in ("A cavity is a set of 1 to CAVMD_SHARED_CAVITY_MAX_MEMBERS items of the object",
                  "Exactly one of them, the carrier, names a photon type (L_typeid >= 0)",
                  "Every other member passes L_typeid = -1", "d_c = sum_i q_i r_i of member c, and D = sum_c d_c",
                  "E_h = 1/2 K q.q, E_c = g (D_xy . q_xy), E_d = 1/2 (g^2/K) D_xy.D_xy", "Dq = q_xy + (g/K) D_xy",
                  "gets ((-g) q_i) Dq in x and y, with z = 0 and w = 0", "The photon gets -K q - g D_xy",
                  "every force of every member of that cavity is zero and its energies are zero",
                  "Other cavities are unaffected", "Members with N == 0 are legal and contribute nothing",
                  "particles base + j 256 + tid, four in flight", "folds the totals of a cavity in ascending item index",
                  "Thread t merges members t, t+256, t+512, t+768, in that order, into an identity accumulator",
                  "come from the carrier's record alone", "all of them hold identical bits of Dq",
                  "no flags, no atomics", "the kernel boundary on the stream orders launch 1 before launch 2",
                  "No member is conserved on its own", "Enqueues exactly TWO kernels"):
        assert words in raw, words


def test_a_c99_program_sees_the_layout_and_the_table_rules(capi, tmp_path):
    out = abi.run_c99("shared_cavity_abi_check", capi, tmp_path)
    assert "SHARED-CAVITY-ABI-OK" in out and "CAVMD_SHARED_CAVITY_MAX_MEMBERS 1024\n" in out
    sizes, offsets = abi.c_layouts(out)
    assert sizes == {"item": 128} and offsets["item"] == OFFSETS
    S = capi.SharedCavityItem
    assert ctypes.sizeof(S) == 128 and {name: getattr(S, name).offset for name, *_ in S._fields_} == OFFSETS
    assert capi.SHARED_CAVITY_MAX_MEMBERS == 1024
    # cavmd_batch_item with the cavity in place of its first reserved word
    B = capi.BatchItem
    shared = {name: getattr(B, name).offset for name, *_ in B._fields_ if name != "reserved"}
    assert shared == {name: off for name, off in OFFSETS.items() if name in shared} and B.reserved.offset == OFFSETS["cavity"]


def test_libraries_export_the_names_and_capi_binds_them(capi):
    paths = [capi.LIB_PATH, capi.HOOKS_LIB_PATH] + [capi.split_variant_path(name) for name in sorted(capi.SPLIT_VARIANTS)]
    assert len(paths) == 5
    for path in paths:
        assert {s for s in abi.exported(path) if s.startswith(PREFIX)} == NAMES, path
    assert NAMES <= set(capi.EXPORTED_SYMBOLS)
    libs = [capi.load(), capi.load_hooks_build()] + [capi.load_split_variant(name) for name in sorted(capi.SPLIT_VARIANTS)]
    for lib in libs:
        for n in NAMES:
            assert getattr(lib, n).restype is ctypes.c_int and getattr(lib, n).argtypes is not None, n
    blob = open(capi.LIB_PATH, "rb").read()
    for kernel in (b"shared_cavity_dipole_kernelILi256E", b"shared_cavity_force_kernelILi256E"):
        assert kernel in blob, kernel
    H = capi.SharedCavity
    assert issubclass(H, capi._ItemTableHandle) and H._PREFIX == "cavmd_shared_cavity" and H._ITEM is capi.SharedCavityItem
    for name in ("compute", "last_sequence", "results", "results_device_ptr", "cell_dipoles_device_ptr", "count", "carrier",
                 "set_items", "close"):
        assert callable(getattr(H, name)), name


def test_null_handles_are_refused(capi):
    INV = capi.CAVMD_ERR_INVALID_VALUE
    byref, vp = ctypes.byref, ctypes.c_void_p
    it = _member(capi, 0, True)
    for lib in (capi.load(), capi.load_hooks_build()):
        out = vp(123)
        assert lib.cavmd_shared_cavity_create(None, 1, byref(it), byref(out)) == INV and not out.value
        assert lib.cavmd_shared_cavity_create(None, 1, byref(it), None) == INV
        assert lib.cavmd_shared_cavity_destroy(None) == 0
        assert lib.cavmd_shared_cavity_set_items(None, 0, 1, byref(it)) == INV
        assert lib.cavmd_shared_cavity_compute(None, None) == INV
        assert lib.cavmd_shared_cavity_last_sequence(None, byref(ctypes.c_uint64())) == INV
        assert lib.cavmd_shared_cavity_results_read(None, None, byref(capi.Result())) == INV
        assert lib.cavmd_shared_cavity_results_device_ptr(None, byref(vp())) == INV
        assert lib.cavmd_shared_cavity_cell_dipoles_device_ptr(None, byref(vp())) == INV
        assert lib.cavmd_shared_cavity_count(None, byref(ctypes.c_uint32())) == INV
        assert lib.cavmd_shared_cavity_carrier(None, 0, byref(ctypes.c_uint32())) == INV
        assert lib.cavmd_shared_cavity_item_check(None) == INV
        assert lib.cavmd_shared_cavity_table_check(1, None, None) == INV


# ---- the table rules ------------------------------------------------------------------------------------------------------------
def _member(capi, cavity, carrier, n=8, params=None):
    return capi.shared_cavity_item(n, 0x10000, 0x20000, 0x30000, 0x40000, (20.0, 21.0, 22.0), 2 if carrier else -1,
                                   params or capi.make_params(0.0091, 1e-3, 1.0), cavity)


def test_every_rule_of_the_table_check(capi):
    OK, INV, CAP, BAD = capi.CAVMD_OK, capi.CAVMD_ERR_INVALID_VALUE, capi.CAVMD_ERR_CAPACITY, capi.CAVMD_ERR_BAD_PARAMS
    check = capi.shared_cavity_table_check
    good = lambda: [_member(capi, 0, True), _member(capi, 1, False), _member(capi, 0, False), _member(capi, 1, True),
                    _member(capi, 2, True, n=0)]
    assert check(good()) == (OK, 3) and check([_member(capi, 0, True)]) == (OK, 1)
    assert check([]) == (INV, None)
    t = good(); t[2].L_typeid = 0                                     # two carriers (any id >= 0 names a photon type)
    assert check(t) == (INV, None)
    t = good(); t[0].L_typeid = -1                                    # none
    assert check(t) == (INV, None)
    t = good(); t[4].cavity = 3                                       # sparse ids: no cavity 2
    assert check(t) == (INV, None)
    t = good(); t[4].cavity = 2 ** 32 - 1
    assert check(t) == (INV, None)
    for field, value in (("couplstr", 2e-3), ("omegac", 0.01), ("K", 1.0), ("phmass", 2.0)):
        t = good(); setattr(t[2].params, field, value)                # differing params
        assert check(t) == (BAD, None), field
    t = good(); t[2].params.phmass = -0.0; t[0].params.phmass = 0.0   # bitwise: -0.0 is not 0.0
    assert check(t) == (BAD, None)
    other = capi.make_params(0.02, 5e-4, 1.0)                          # but cavities need not agree with each other
    t = good(); t[1].params = other; t[3].params = other
    assert check(t) == (OK, 3)
    # the rows' own rules, cavmd_batch_item_check's
    t = good(); t[1].reserved0 = 1
    assert check(t) == (INV, None) and capi.shared_cavity_item_check(t[1]) == INV
    t = good(); t[1].reserved[2] = 1
    assert check(t) == (INV, None)
    t = good(); t[1].d_pos = 0x10008
    assert check(t) == (INV, None)
    t = good(); t[1].N = capi.BATCH_MAX_ITEM_N + 1
    assert check(t) == (CAP, None)
    t = good(); t[1].params.K = 0.0; t[3].params.K = 0.0
    assert check(t) == (BAD, None) and capi.shared_cavity_item_check(t[1]) == BAD
    empty = capi.shared_cavity_item(0, 0, 0, 0, 0, (0.0, 0.0, 0.0), -1, t[0].params, 0)
    assert capi.shared_cavity_item_check(empty) == OK and check(good() + [empty]) == (OK, 3)
    # the cap
    full = [_member(capi, 0, k == 1023) for k in range(1024)]
    assert check(full) == (OK, 1)
    assert check(full + [_member(capi, 0, False)]) == (CAP, None)
    assert check(full + [_member(capi, 1, True)]) == (OK, 2)


def test_the_python_class_is_exported_and_refuses_cpu_tensors(capi):
    import cavitymd
    from cavitymd import synthetic
    assert "SharedCavityForceBatch" in cavitymd.__all__ and cavitymd.SharedCavityForceBatch is cavitymd.shared_cavity.SharedCavityForceBatch
    cls = cavitymd.SharedCavityForceBatch
    for name in ("compute", "energies", "results", "refresh", "close", "last_sequence"):
        assert callable(getattr(cls, name)), name
    for name in ("forces", "cell_dipoles", "carriers", "batch", "n_cavities"):
        assert isinstance(getattr(cls, name), property), name
    cfg = synthetic.config1()
    pd = cavitymd.ParticleData.from_arrays(cfg["position"], cfg["typeid"], cfg["charge"], cfg["image"], cfg["types"], cfg["box"],
                                           device="cpu")
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        cls([cavitymd.SystemDefinition(pd)], [0], cfg["params"])
