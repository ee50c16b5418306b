"""GPU: mzk_plonk_wire_permutation_dev (include/mzk.h; csrc/perm.cuh) -- next[] of a variable table must be, integer for integer, the
cycle of compute_wire_permutation (relation/src/constraint_system.rs:743-778) as oracle/pyref_circuit.py:55-63 restates it: the
occurrence list of every variable in cell order, each cell linked to the one after it and the last to the first.
Sizes: one cell; 63 / 64 / 65 (a wavefront and its neighbours); 257 (a tile of 256 and one); 40 (n = 8, W = 5); 300007 (more cells than
1024 tiles: every block walks two tiles, the last block a partial one); 4096 and 81920 cells under variable counts on both sides of the
8-bit digit boundaries (1, 2 and 3 passes)."""
import ctypes as C
from functools import lru_cache

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
INVALID, UNSUPPORTED = -1, -5


def expected_next(var, n_vars):
    """oracle/pyref_circuit.py:55-63 on flat cells"""
    occ = [[] for _ in range(n_vars)]
    for cell, v in enumerate(var.tolist()):
        occ[v].append(cell)
    nxt = [0] * len(var)
    for lst in occ:
        for q, cell in enumerate(lst):
            nxt[cell] = lst[(q + 1) % len(lst)]
    return np.array(nxt, dtype=np.uint32)


def device_next(lib, var, n_vars):
    """-> (return code, next[] as uint32, raw bytes)"""
    import torch
    L = lib.load()
    d_var = torch.from_numpy(np.array(var, dtype=np.uint32).view(np.int32)).cuda()
    d_next = torch.full((max(len(var), 1),), -1, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    rc = L.mzk_plonk_wire_permutation_dev(C.c_void_p(d_var.data_ptr()), len(var), n_vars, C.c_void_p(d_next.data_ptr()), None)
    out = d_next.cpu().numpy()[:len(var)].view(np.uint32)
    return rc, out, out.tobytes()


@lru_cache(maxsize=None)
def random_table(cells, n_vars, seed):
    """random assignment over roughly the lower 3/4 of the indices, so that some are unused, plus the highest index once"""
    rng = np.random.default_rng(seed)
    var = rng.integers(0, max(1, (3 * n_vars) // 4), size=cells, dtype=np.uint32)
    var[cells // 2] = n_vars - 1
    var.setflags(write=False)
    return var, expected_next(var, n_vars)


@pytest.mark.parametrize("cells", [1, 63, 64, 65, 257, 40, 300007])
def test_random_tables_of_every_size(gpu, cells):
    n_vars = max(1, cells // 3)
    var, want = random_table(cells, n_vars, 100 + cells)
    rc, got, _ = device_next(gpu, var, n_vars)
    assert rc == 0 and np.array_equal(got, want)


@pytest.mark.parametrize("cells", [1, 65, 257, 4099])
def test_all_distinct_is_the_identity_and_one_variable_is_one_cycle(gpu, cells):
    rc, got, _ = device_next(gpu, np.arange(cells, dtype=np.uint32)[::-1].copy(), cells)           # distinct, in descending order
    assert rc == 0 and np.array_equal(got, np.arange(cells, dtype=np.uint32))
    for n_vars, v in ((1, 0), (cells + 7, cells + 6)):                                                # no pass at all / every pass, one digit value each
        rc, got, _ = device_next(gpu, np.full(cells, v, dtype=np.uint32), n_vars)
        assert rc == 0 and np.array_equal(got, (np.arange(cells, dtype=np.uint32) + 1) % cells)


@pytest.mark.parametrize("n_vars,cells", [(1, 4096), (255, 4096), (256, 4096), (257, 4096), (65535, 81920), (65536, 81920), (65537, 81920)])
def test_digit_boundaries(gpu, n_vars, cells):
    var, want = random_table(cells, n_vars, 7 * n_vars)
    rc, got, _ = device_next(gpu, var, n_vars)
    assert rc == 0 and np.array_equal(got, want)


def test_one_variable_on_most_cells_and_the_same_bytes_twice(gpu):
    """60 % of 5 * 2^12 cells on variable 0 (the bench circuit's `zero`), the rest random: the heavy run crosses most blocks"""
    cells, n_vars = 5 << 12, 3000
    rng = np.random.default_rng(5)
    var = rng.integers(1, n_vars, size=cells, dtype=np.uint32)
    var[rng.permutation(cells)[:(6 * cells) // 10]] = 0
    want = expected_next(var, n_vars)
    rc, got, raw = device_next(gpu, var, n_vars)
    assert rc == 0 and np.array_equal(got, want)
    rc, _, again = device_next(gpu, var, n_vars)
    assert rc == 0 and again == raw


def test_an_index_outside_the_variables_is_refused_with_its_lowest_cell(gpu):
    L = gpu.load()
    cells, n_vars = 5000, 300
    var = np.random.default_rng(9).integers(0, n_vars, size=cells, dtype=np.uint32)
    var[777] = n_vars
    var[4000] = n_vars + 5
    rc, _, _ = device_next(gpu, var, n_vars)
    msg = L.mzk_last_error().decode()
    assert rc == INVALID and "cell 777 " in msg and "index %d " % n_vars in msg, msg
    var[777] = 0
    rc, _, _ = device_next(gpu, var, n_vars)
    assert rc == INVALID and "cell 4000 " in L.mzk_last_error().decode()
    var[4000] = 0
    assert device_next(gpu, var, n_vars)[0] == 0
    assert device_next(gpu, var, 0)[0] == INVALID
    # 2^32 cells and more are refused before anything is read
    import torch
    t = torch.zeros(4, dtype=torch.int32, device="cuda")
    assert L.mzk_plonk_wire_permutation_dev(C.c_void_p(t.data_ptr()), 1 << 32, 5, C.c_void_p(t.data_ptr()), None) == UNSUPPORTED
