"""The lane-split builds of the library (csrc/Makefile's `split_variants`, cavitymd._capi.load_split_variant) on a machine
WITHOUT a GPU: with the product library they answer cavmd_molecular_order and cavmd_coulomb_order with the table below, the
union of their answers is exactly what include/cavmd.h allows, they export what the product exports, and the splits do not
leak into the host arithmetic.  tests/test_gpu_split_variants.py runs their kernels; the shapes it uses (tests/split_builds.py) are checked here."""
import ctypes
import os
import re

import pytest

import coulomb_mirror as mirror
from abi_support import HEADER, exported
from abi_support import good_coulomb as _good
from split_builds import BUILDS, k_counts_for, k_values_for, replay_k_counts, sizes_for


@pytest.fixture(scope="module")
def libs(capi):
    return {name: capi.load() if name == "product" else capi.load_split_variant(name) for name in BUILDS}


def _paths(capi):
    return {name: capi.LIB_PATH if name == "product" else capi.split_variant_path(name) for name in BUILDS}


def _allowed(define):
    """the values the header's comment on `define` allows: '#ifndef CAVMD_..._SPLIT   /* S, one of 1, 4, 16: ...'"""
    line = re.search(rf"^#ifndef\s+{define}\s*/\*\s*[ST], one of ([\d, ]+)[:;]", open(HEADER).read(), flags=re.M)
    assert line, define
    return {int(v) for v in line.group(1).split(",")}


def test_every_build_answers_its_row_of_the_table(capi, libs):
    assert capi.SPLIT_VARIANTS == {name: splits for name, splits in BUILDS.items() if name != "product"}
    for name, (S_mol, S, T) in BUILDS.items():
        assert capi.molecular_order(libs[name]) == (256 // S_mol, S_mol), name
        assert capi.coulomb_order(libs[name]) == (256 // S, S, 256 // T, T), name
    assert capi.molecular_order() == capi.molecular_order(libs["product"])       # without a library: the product's
    assert len({id(lib) for lib in libs.values()}) == 4 and capi.load_split_variant("a") is libs["a"]
    with pytest.raises(ValueError):
        capi.load_split_variant("d")
    for define, column in (("CAVMD_MOLECULAR_J_SPLIT", 0), ("CAVMD_COULOMB_J_SPLIT", 1), ("CAVMD_COULOMB_K_SPLIT", 2)):
        assert re.search(rf"#define\s+{define}\s+{BUILDS['product'][column]}\b", open(HEADER).read()), define


def test_the_builds_cover_exactly_what_the_header_allows(capi, libs):
    assert _allowed("CAVMD_MOLECULAR_J_SPLIT") == {1, 4, 16}
    assert _allowed("CAVMD_COULOMB_J_SPLIT") == _allowed("CAVMD_COULOMB_K_SPLIT") == {1, 4, 16, 64}
    assert {capi.molecular_order(lib)[1] for lib in libs.values()} == _allowed("CAVMD_MOLECULAR_J_SPLIT")
    assert {capi.coulomb_order(lib)[1] for lib in libs.values()} == _allowed("CAVMD_COULOMB_J_SPLIT")
    assert {capi.coulomb_order(lib)[3] for lib in libs.values()} == _allowed("CAVMD_COULOMB_K_SPLIT")


def test_the_variants_export_what_the_product_exports(capi):
    symbols = {}
    for name, path in _paths(capi).items():
        symbols[name] = {s for s in exported(path) if s.startswith("cavmd_")}
        assert b"gfx950" in open(path, "rb").read(), name
    assert symbols["product"] == set(capi.EXPORTED_SYMBOLS)
    for name in ("a", "b", "c"):
        assert symbols[name] == symbols["product"], name


def _k_count(lib, item):
    K = ctypes.c_uint32()
    status = lib.cavmd_coulomb_k_count(ctypes.byref(item), ctypes.byref(K))
    return status, int(K.value)


def test_the_splits_do_not_leak_into_the_host_arithmetic(capi, libs):
    items = [_good(capi), _good(capi, 4), _good(capi, 2048), _good(capi, 2049), _good(capi, k_cut=0.0), _good(capi, k_cut=1e9),
             _good(capi, kappa=0.0), _good(capi, exclusions=((0, 501),)), _good(capi, 64, (), (4.0, 4.0, 4.0), 2.0, 2.0, 18.209),
             capi.coulomb_item(0, 0, 0, 0, (0.0, 0.0, 0.0), 0.0, 0.0, 0.0)]
    for K in (0, 1, 2, 63, 64, 65, 300, 4096, 4097):
        box, k_cut = mirror.box_and_k_cut_for((8.0, 9.0, 10.0), K)
        items.append(_good(capi, box=box, k_cut=k_cut))
    answers = {name: [(lib.cavmd_coulomb_item_check(ctypes.byref(it)),) + _k_count(lib, it) for it in items]
               for name, lib in libs.items()}
    assert answers["product"][0] == (0, 0, len(mirror.k_vectors((8.0, 9.0, 10.0), 3.0)[2]))
    assert [a[0] for a in answers["product"][:10]] == [0, 0, 0, capi.CAVMD_ERR_CAPACITY, 0, capi.CAVMD_ERR_CAPACITY,
                                                       capi.CAVMD_ERR_INVALID_VALUE, capi.CAVMD_ERR_INVALID_VALUE, 0, 0]
    assert [a[2] for a in answers["product"][10:18]] == [0, 1, 2, 63, 64, 65, 300, 4096]
    for name in ("a", "b", "c"):
        assert answers[name] == answers["product"], name


def test_every_shape_of_the_gpu_tests_exists_at_every_split(capi, libs):
    """tests/test_gpu_split_variants.py pairs N and K on each build's own boundaries; a k_cut reaches a count only where a
    shell of k2 ends, so each K needs a box (mirror.box_and_k_cut_for raises where it finds none).  Every K of every build has
    one, for both base boxes of the ragged systems, and every library counts it as the mirror does."""
    for name, lib in libs.items():
        ROWS, S, KROWS, T = capi.coulomb_order(lib)
        for rows in (ROWS, capi.molecular_order(lib)[0]):
            sizes = sizes_for(rows)
            assert len(set(sizes)) == len(sizes) and min(sizes) == 0 and sum(1 for n in sizes if n > 19) >= 2
            assert {rows - 1, rows, rows + 1, 2 * rows + 1, 63, 64, 65, 501} <= set(sizes)
        sizes = sizes_for(ROWS)
        counts = k_counts_for(sizes, KROWS)
        assert set(counts) == set(k_values_for(KROWS)) == {0, 1, KROWS - 1, KROWS, KROWS + 1, 2 * KROWS + 1, 300}
        start, smaller, larger = replay_k_counts(KROWS)
        assert smaller <= KROWS and -(-larger // KROWS) >= -(-start[1] // KROWS) + 2
        wanted = [(k, K) for k, (n, K) in enumerate(zip(sizes, counts)) if n > 0]
        wanted += [(k, K) for k, K in enumerate(start)] + [(1, smaller), (1, larger)]
        for k, K in wanted:
            box, k_cut = mirror.box_and_k_cut_for((8.0, 10.0 + 2.0 * (k % 2), 16.0), K)
            assert min(box) * 0.5 >= 3.0                                         # the GPU tests' r_cut
            assert _k_count(lib, _good(capi, 40, (), box, 1.0, 3.0, k_cut)) == (0, K) and len(mirror.k_vectors(box, k_cut)[2]) == K


def test_a_second_build_does_nothing(capi):
    paths = list(_paths(capi).values()) + [capi.HOOKS_LIB_PATH]
    before = [os.stat(p).st_mtime_ns for p in paths]
    capi.build()
    assert [os.stat(p).st_mtime_ns for p in paths] == before
    makefile = open(os.path.join(capi.CSRC_DIR, "Makefile")).read()
    clean = makefile[makefile.index("\nclean:"):]
    assert "split_variants:" in makefile and "$(SPLIT_VARIANTS)" in clean
