"""The lane-split builds of the library and the shapes their tests use: tests/test_gpu_split_variants.py runs the kernels at
these sizes, tests/test_split_variants_abi.py checks without a GPU that every one of them exists at every split."""

# build -> (CAVMD_MOLECULAR_J_SPLIT, CAVMD_COULOMB_J_SPLIT, CAVMD_COULOMB_K_SPLIT): the product library and csrc/Makefile's
# split_variants
BUILDS = {"product": (16, 16, 4), "a": (1, 1, 1), "b": (4, 4, 16), "c": (16, 64, 64)}


def _distinct(values):
    out = []
    for v in values:
        if v >= 0 and v not in out:
            out.append(v)
    return tuple(out)


def sizes_for(rows):
    """N on the boundaries of a workgroup of `rows` particles, the wave (64: also the S = 64 group) and the production system
    (501, which carries every planted edge)"""
    return _distinct((0, 1, 2, rows - 1, rows, rows + 1, 2 * rows + 1, 63, 64, 65, 501))


def k_values_for(k_rows):
    """K on the boundaries of a workgroup of `k_rows` k-vectors.  mirror.box_and_k_cut_for finds a box for every one of them,
    at all four KROWS and for both base boxes of coulomb_ragged.ragged_system (test_split_variants_abi.py checks it against each library's
    own count), so none is replaced by a neighbour."""
    return _distinct((0, 1, k_rows - 1, k_rows, k_rows + 1, 2 * k_rows + 1, 300))


def k_counts_for(sizes, k_rows):
    """the K values cycled over the items"""
    values = k_values_for(k_rows)
    return tuple(values[i % len(values)] for i in range(len(sizes)))


def replay_k_counts(k_rows):
    """K of the three items of the replay tests (two, three and one workgroup of launch 1), what item 1 shrinks to (one
    workgroup) and what it grows to (at least two workgroups more than it was captured with)"""
    grown = 300 if 300 > 3 * k_rows else 4 * k_rows + 1
    return (k_rows + 1, 2 * k_rows + 1, k_rows - 1), k_rows, grown
