"""GPU: from sigma back to the wire-variable table (include/mzk.h; csrc/unperm.cuh) -- mzk_plonk_sigma_decode_dev,
mzk_plonk_variables_from_permutation_dev, mzk_prover_derive_wire_variables, mzk_prover_get_wire_variables.  The expected table is always
computed on the CPU (tests/check_witness_ref.py::wire_variables_from_sigma, or `canon` / `label` below), never by the code under test,
and compared exactly.
Sizes of the primitives: 40 cells (W = 5, n = 8: a partial wave), 6 x 64, 5 x 2^10 (one cycle of all 5120 cells is 13 rounds across 20
workgroups), 5 x 2^16 (a seeded random partition: the scans cross 1280 workgroups).  Handles: log_n 3, 6, 9, 12, both circuit types and
curves, built from coefficient forms -- the path that has no table."""
import ctypes as C
import random
import re
from functools import lru_cache

import numpy as np
import pytest

import check_witness_ref as REF
from test_check_witness_gpu import _check, _instance, _limbs, _prove
from test_derive_variables import canon

pytestmark = pytest.mark.gpu
INVALID, BAD_HANDLE, UNSUPPORTED = -1, -4, -5
LENGTHS = (1, 2, 3, 63, 64, 65, 255, 256, 257)


def label(nxt):
    """cycles of a permutation in canonical numbering: scanning the cells in order, the first unseen cell names the next variable"""
    nxt = [int(x) for x in nxt]
    var = [-1] * len(nxt)
    n_vars = 0
    for c in range(len(nxt)):
        if var[c] >= 0:
            continue
        a = c
        while var[a] < 0:
            var[a] = n_vars
            a = nxt[a]
        n_vars += 1
    return np.array(var, dtype=np.uint32), n_vars


def from_cycles(cells, cycles):
    """next[] with the given cycles (each a list of cells, in the order they follow each other); every other cell is a fixed point"""
    nxt = np.arange(cells, dtype=np.uint32)
    for cyc in cycles:
        for q, c in enumerate(cyc):
            nxt[c] = cyc[(q + 1) % len(cyc)]
    return nxt


@lru_cache(maxsize=None)
def permutation(kind, W, n):
    """-> (next, expected variables, expected n_vars), read-only"""
    cells = W * n
    rng = random.Random(31 * cells + len(kind))
    if kind == "identity":
        nxt = np.arange(cells, dtype=np.uint32)
    elif kind == "one cycle":
        nxt = (np.arange(cells, dtype=np.uint32) + 1) % cells
    elif kind == "one cycle, reversed":
        nxt = (np.arange(cells, dtype=np.uint32) + cells - 1) % cells
    elif kind == "one cycle, shuffled":                                   # crosses wires at every step
        order = list(range(cells))
        rng.shuffle(order)
        nxt = from_cycles(cells, [order])
    elif kind == "lengths side by side":                                  # 1, 2, 3, 63, .. 257 on consecutive cells, as many as fit, repeated
        cycles, at = [], 0
        while at < cells:
            for m in LENGTHS:
                m = min(m, cells - at)
                if m:
                    cycles.append(list(range(at, at + m)))
                    at += m
        nxt = from_cycles(cells, cycles)
    elif kind == "across wires":                                          # row j of every wire in one cycle, the wires in an order of its own per row
        cycles = []
        for j in range(n):
            wires = list(range(W))
            rng.shuffle(wires)
            cycles.append([w * n + j for w in wires])
        nxt = from_cycles(cells, cycles)
    elif kind == "random partition":                                      # seeded lengths (small ones, the listed ones, a few long ones) over shuffled cells
        order = list(range(cells))
        rng.shuffle(order)
        cycles, at = [], 0
        while at < cells:
            m = min(rng.choice((1, 1, 2, 3, 5, 17) + LENGTHS + (1000, 4097, 30011)), cells - at)
            cycles.append(order[at:at + m])
            at += m
        nxt = from_cycles(cells, cycles)
    else:
        raise AssertionError(kind)
    var, n_vars = label(nxt)
    nxt.setflags(write=False)
    var.setflags(write=False)
    return nxt, var, n_vars


def device_label(mj, nxt):
    import torch
    d = torch.from_numpy(np.array(nxt, dtype=np.uint32).view(np.int32)).cuda()
    out, n_vars = mj.plonk.variables_from_permutation(d)
    return out.cpu().numpy().view(np.uint32), n_vars


KINDS = ("identity", "one cycle", "one cycle, reversed", "one cycle, shuffled", "lengths side by side", "across wires")


@pytest.mark.parametrize("W,n", [(5, 8), (6, 64), (5, 1 << 10)])
@pytest.mark.parametrize("kind", KINDS)
def test_hand_built_permutations(gpu, mj, kind, W, n):
    nxt, want, want_n = permutation(kind, W, n)
    got, n_vars = device_label(mj, nxt)
    assert n_vars == want_n and np.array_equal(got, want)
    if kind == "identity":
        assert n_vars == W * n
    if kind.startswith("one cycle"):
        assert n_vars == 1 and not got.any()


@pytest.mark.parametrize("kind", ["random partition", "lengths side by side", "one cycle, shuffled"])
def test_many_workgroups(gpu, mj, kind):
    nxt, want, want_n = permutation(kind, 5, 1 << 16)
    got, n_vars = device_label(mj, nxt)
    assert n_vars == want_n and np.array_equal(got, want)
    again, n_again = device_label(mj, nxt)                                 # a function of the input alone
    assert n_again == n_vars and again.tobytes() == got.tobytes()


def test_what_is_no_permutation_is_refused_with_its_lowest_cell(gpu, mj):
    import torch
    L = gpu.load()
    cells = 5 * 64
    base = permutation("across wires", 5, 64)[0]

    def run(nxt, count=cells):
        d = torch.from_numpy(np.array(nxt, dtype=np.uint32).view(np.int32)).cuda()
        out = torch.zeros(max(count, 1), dtype=torch.int32, device="cuda")
        n_vars = C.c_uint64(77)
        torch.cuda.synchronize()
        rc = L.mzk_plonk_variables_from_permutation_dev(C.c_void_p(d.data_ptr()), count, C.c_void_p(out.data_ptr()), C.byref(n_vars), None)
        return rc, L.mzk_last_error().decode()

    bad = np.array(base)
    bad[200], bad[70] = cells, cells + 5                                   # two entries out of range: the lower cell is named
    rc, msg = run(bad)
    assert rc == INVALID and re.search(r"cell 70 holds %d\b" % (cells + 5), msg), msg
    bad = np.array(base)
    lost = sorted((int(base[130]), int(base[9])))
    bad[130] = bad[9] = base[17]                                           # three cells on one successor: two cells lose their predecessor
    rc, msg = run(bad)
    assert rc == INVALID and re.search(r"cell %d is the successor of no cell" % lost[0], msg), msg
    assert run(base)[0] == 0 and run(base, 0)[0] == 0                      # (no cells: nothing to do)
    assert L.mzk_plonk_variables_from_permutation_dev(None, 1 << 32, None, C.byref(C.c_uint64()), None) == UNSUPPORTED
    assert L.mzk_plonk_variables_from_permutation_dev(None, 8, None, C.byref(C.c_uint64()), None) == INVALID


# ---- table -> permutation -> sigma -> permutation -> table ---------------------------------------------------------------------------
@pytest.mark.parametrize("curve_id,W,log_n", [(0, 5, 6), (1, 6, 6), (1, 5, 10), (0, 6, 10)])
def test_round_trip_through_the_forward_primitives(gpu, mj, curve_id, W, log_n):
    import torch
    L = gpu.load()
    c = mj.params.CURVES[curve_id]
    n = 1 << log_n
    cells = W * n
    rng = np.random.default_rng(40 + curve_id + log_n)
    n_vars = cells // 3
    table = rng.integers(0, n_vars, size=(W, n), dtype=np.uint32)
    table[W - 1, n - 5:] = 1                                               # a run at the very end, and one variable on many cells
    table.reshape(-1)[rng.permutation(cells)[:cells // 4]] = 0
    k = mj.rng.compute_coset_representatives(c, W, n)
    kk = mj.params.fr_to_mont(c, k)
    d_var = torch.from_numpy(table.view(np.int32)).cuda()
    d_next = torch.empty((W, n), dtype=torch.int32, device="cuda")
    d_sig = torch.empty((W, n, 4), dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    gpu.check(L.mzk_plonk_wire_permutation_dev(C.c_void_p(d_var.data_ptr()), cells, n_vars, C.c_void_p(d_next.data_ptr()), None), "perm")
    gpu.check(L.mzk_plonk_sigma_values_dev(c.curve_id, log_n, W, C.c_void_p(d_next.data_ptr()), C.c_void_p(kk.ctypes.data), C.c_void_p(d_sig.data_ptr()), None), "sigma")
    gpu.check(L.mzk_dev_sync(), "sync")
    back = mj.plonk.sigma_decode(c, d_sig, k)
    assert torch.equal(back, d_next)
    got, got_n = mj.plonk.variables_from_permutation(back)
    want, want_n = canon(table)
    assert got_n == want_n and np.array_equal(got.cpu().numpy().view(np.uint32), np.array(want, dtype=np.uint32))


def test_sigma_decode_names_the_lowest_cell_that_is_no_identity_value(gpu, mj):
    import torch
    L = gpu.load()
    c = mj.params.CURVES[0]
    W, log_n = 5, 6
    n = 1 << log_n
    k = mj.rng.compute_coset_representatives(c, W, n)
    kk = mj.params.fr_to_mont(c, k)
    dom = mj.Radix2EvaluationDomain(c, log_n)
    w_n = mj.params.fr_from_mont(c, dom.fft(mj.params.fr_to_mont(c, [0, 1] + [0] * (n - 2))))[1]      # X on H: the NTT's own root
    ident = [[ka * pow(w_n, b, c.r) % c.r for b in range(n)] for ka in k]
    run = lambda sig, kmont=kk: (L.mzk_plonk_sigma_decode_dev(0, log_n, W, C.c_void_p(sig.data_ptr()), C.c_void_p(kmont.ctypes.data), C.c_void_p(out.data_ptr()), None),
                                 L.mzk_last_error().decode())
    out = torch.empty((W, n), dtype=torch.int32, device="cuda")
    up = lambda rows: torch.from_numpy(np.stack([mj.params.fr_to_mont(c, r) for r in rows]).view(np.int64)).cuda()
    rc, _ = run(up(ident))
    assert rc == 0 and np.array_equal(out.cpu().numpy().reshape(-1), np.arange(W * n))
    bad = [row[:] for row in ident]
    bad[3][7] = (bad[3][7] + 1) % c.r
    bad[1][2] = 12345
    rc, msg = run(up(bad))
    assert rc == INVALID and "cell %d: not k_a w^b" % (1 * n + 2) in msg, msg
    # cosets that are not disjoint: k_2 = k_0 w^3 -- the identity values of wire 2 are those of wire 0
    k2 = list(k)
    k2[2] = k[0] * pow(w_n, 3, c.r) % c.r
    rc, msg = run(up(ident), mj.params.fr_to_mont(c, k2))
    assert rc == INVALID and "not disjoint" in msg and re.search(r"cell (\d+)", msg).group(1) == "0", msg
    assert L.mzk_plonk_sigma_decode_dev(0, 30, 5, C.c_void_p(out.data_ptr()), C.c_void_p(kk.ctypes.data), C.c_void_p(out.data_ptr()), None) == UNSUPPORTED
    assert L.mzk_plonk_sigma_decode_dev(0, log_n, 4, C.c_void_p(out.data_ptr()), C.c_void_p(kk.ctypes.data), C.c_void_p(out.data_ptr()), None) == INVALID


# ---- handles created from coefficient forms --------------------------------------------------------------------------------------------
def _cells_by_variable(wv, n):
    by = {}
    for i, col in enumerate(wv):
        for j, v in enumerate(col):
            by.setdefault(v, []).append(i * n + j)
    return by


HANDLES = [(0, False, 3), (1, False, 6), (0, False, 9), (1, False, 12), (1, True, 4), (0, True, 6), (1, True, 9), (0, True, 12)]


@pytest.mark.parametrize("curve_id,ultra,log_n", HANDLES)
def test_derive_get_and_the_copy_family_of_check_witness(gpu, mj, curve_id, ultra, log_n):
    import torch
    inst = _instance(mj, curve_id, ultra, log_n, "hot", 2 if log_n == 4 else 3)
    n, W, r, native = inst.n, inst.W, inst.c.r, inst.native
    wv, n_vars = REF.wire_variables_from_sigma(inst.pc, inst.sig, inst.k, log_n)
    assert not native.check_witness(_limbs(inst, inst.w), inst.pub).copy_checked
    assert native.derive_wire_variables() == n_vars
    table, got_n = native.wire_variables()
    assert got_n == n_vars and table.dtype == np.uint32 and np.array_equal(table, np.array(wv, dtype=np.uint32))
    by = _cells_by_variable(wv, n)
    longest = max(by.values(), key=len)
    some = next(cells for cells in by.values() if len(cells) >= 2)
    cases = [[], [some[0]], [some[-1]], [longest[0]], [longest[len(longest) // 2], some[-1], W * n - 1]]
    if ultra and log_n >= 9:                                               # (the lookup wire's value classes; TurboPlonk cycles have 3 cells)
        assert len(longest) > 64
    dev = lambda w: torch.from_numpy(_limbs(inst, w).view(np.int64)).cuda()
    for cells in cases:
        bad = [col[:] for col in inst.w]
        for cell in cells:
            bad[cell // n][cell % n] = (bad[cell // n][cell % n] + 1 + cell) % r
        for wires in (dev(bad), _limbs(inst, bad)):                        # MZK_WITNESS_DEV_WIRES, MZK_WITNESS_HOST_WIRES
            rep = native.check_witness(wires, inst.pub)
            exp = _check(inst, rep, bad, wire_vars=wv)
            assert rep.copy_checked and bool(exp["copy"]) == bool(cells)
    inst.release()


@pytest.mark.parametrize("curve_id", [0, 1])
def test_two_variables_own_most_cells(gpu, mj, curve_id):
    """the bench circuit: `zero` sits on every unused cell and `one` on wire 1 of every addition"""
    c = mj.params.CURVES[curve_id]
    cs = mj.snark.gen_circuit_for_bench(c, 1 << 10, "UltraPlonk")
    assert cs.n == 1 << 10
    ck = mj.UnivariateProverParam.gen_srs_for_testing(c, 77, cs.n + 2)
    pk = mj.snark.preprocess(ck, cs)                                       # from coefficient forms: no table
    var = cs.wire_variables.cpu().numpy()
    counts = np.bincount(var.reshape(-1))
    assert counts[0] + counts[1] > 3 * cs.n
    want, want_n = canon(var.tolist())
    assert pk.derive_wire_variables() == want_n
    table, n_vars = pk.wire_variables()
    assert n_vars == want_n and np.array_equal(table, np.array(want, dtype=np.uint32))
    pk.release()
    ck.release()


@pytest.mark.parametrize("curve_id,ultra", [(0, False), (1, True)])
def test_vector_kinds_prove_from_the_canonical_witness_vector(gpu, mj, curve_id, ultra):
    import torch
    inst = _instance(mj, curve_id, ultra, 6)
    n, native = inst.n, inst.native
    wires = _limbs(inst, inst.w)
    want = _prove(mj, inst, torch.from_numpy(wires.view(np.int64)).cuda())
    # no table yet: the vector kinds are refused
    assert gpu.load().mzk_prover_check_witness(native.handle, 2, C.c_void_p(wires.ctypes.data), 7, None, None, 0, C.byref(gpu.WitnessReport())) == INVALID
    n_vars = native.derive_wire_variables()
    table, _ = native.wire_variables()
    flat = table.reshape(-1)
    first = np.full(n_vars, -1, dtype=np.int64)
    for cell in range(flat.shape[0] - 1, -1, -1):
        first[flat[cell]] = cell                                           # the smallest cell of every variable: the minimum of its cycle
    assert (first >= 0).all() and np.array_equal(np.sort(first), first)
    vec = np.ascontiguousarray(wires.reshape(-1, 4)[first])
    hw = mj.snark.HostWitness(vec, table)
    rep = native.check_witness(hw, inst.pub)
    assert rep.satisfied and rep.copy_checked
    assert _prove(mj, inst, hw) == want
    assert _prove(mj, inst, mj.snark.HostWitness(torch.from_numpy(vec.view(np.int64)).cuda(), table)) == want       # MZK_WITNESS_DEV_VECTOR
    inst.release()


def test_forks_replacement_and_memory(gpu, mj):
    inst = _instance(mj, 0, False, 6)
    n, W, native = inst.n, inst.W, inst.native
    wires = _limbs(inst, inst.w)
    wv, n_vars = REF.wire_variables_from_sigma(inst.pc, inst.sig, inst.k, 6)
    want = np.array(wv, dtype=np.uint32)
    # a fork derives for itself alone (copy-on-write); the table counts in its workspace
    fork = native.fork()
    before = fork.hbm_bytes()
    assert fork.derive_wire_variables() == n_vars
    after = fork.hbm_bytes()
    assert after["prover_workspace"] - before["prover_workspace"] == W * n * 4
    assert {k: v for k, v in after.items() if k != "prover_workspace"} == {k: v for k, v in before.items() if k != "prover_workspace"}
    assert fork.check_witness(wires, inst.pub).copy_checked and not native.check_witness(wires, inst.pub).copy_checked
    with pytest.raises(Exception):
        native.wire_variables()
    assert np.array_equal(fork.wire_variables()[0], want)
    fork.release()
    # alone again, the handle derives into its key; a later fork has the table
    hb = native.hbm_bytes()
    assert native.derive_wire_variables() == n_vars and native.hbm_bytes()["prover_workspace"] - hb["prover_workspace"] == W * n * 4
    late = native.fork()
    assert np.array_equal(late.wire_variables()[0], want) and late.check_witness(wires, inst.pub).copy_checked
    late.release()
    # a table in another numbering is replaced by the canonical one
    names = np.random.default_rng(3).permutation(2 * n_vars)[:n_vars].astype(np.uint32)
    native.set_wire_variables(names[want], 2 * n_vars)
    got, got_n = native.wire_variables()
    assert got_n == 2 * n_vars and np.array_equal(got, names[want])
    assert native.derive_wire_variables() == n_vars and np.array_equal(native.wire_variables()[0], want)
    inst.release()


def test_derive_on_a_prover_from_circuit_structure_gives_the_canonical_table(gpu, mj):
    c = mj.params.CURVES[1]
    cs = mj.snark.gen_circuit_for_bench(c, 100, "TurboPlonk", dense_seed=9)
    ck = mj.UnivariateProverParam.gen_srs_for_testing(c, 78, cs.n + 2)
    pk = mj.snark.preprocess(ck, cs, from_structure=True)
    var = cs.wire_variables.cpu().numpy()
    got, got_n = pk.wire_variables()
    assert got_n == int(cs.witness.shape[0]) and np.array_equal(got, var.astype(np.uint32))
    want, want_n = canon(var.tolist())
    assert pk.derive_wire_variables() == want_n
    got, got_n = pk.wire_variables()
    assert got_n == want_n and np.array_equal(got, np.array(want, dtype=np.uint32))
    assert pk.check_witness(cs.wire_values, []).satisfied
    pk.release()
    ck.release()


def _outcome(mj, inst, wires):
    try:
        return _prove(mj, inst, wires)
    except mj.plonk.PlonkError as e:
        return e.kind


def test_errors_leave_the_handle_as_it_was(gpu, mj):
    """sigma polynomials that are not those of a permutation: one value that is no k_a w^b; two cells with one successor.  A proof on
    such a key ends as it did before the call (its permutation argument cannot close: WrongQuotientPolyDegree)."""
    import types
    L = gpu.load()
    base = _instance(mj, 1, False, 6)
    c, n, W, r = base.c, base.n, base.W, base.c.r
    dom = mj.Radix2EvaluationDomain(c, 6)
    from conftest import fr_mont_limbs
    wv, n_vars = REF.wire_variables_from_sigma(base.pc, base.sig, base.k, 6)
    cell_of = {}
    w_n = base.pc.root_of_unity(6)
    for a in range(W):
        for b in range(n):
            cell_of[base.k[a] * pow(w_n, b, r) % r] = a * n + b
    wires = _limbs(base, base.w)
    want = _prove(mj, base, wires)

    def with_sigma(sig):
        native = mj.prover.TurboPlonkProver(c, n, [dom.ifft(fr_mont_limbs(c, s)) for s in base.sel], [dom.ifft(fr_mont_limbs(c, s)) for s in sig], base.k, base.ck)
        return types.SimpleNamespace(c=c, native=native, pub=base.pub, blind=base.blind)

    # (a) cells 1 n + 5 and 3 n + 9 hold values that are no identity value
    sig = [row[:] for row in base.sig]
    sig[3][9] = (sig[3][9] + 1) % r
    sig[1][5] = 987654321
    assert sig[3][9] not in cell_of and sig[1][5] not in cell_of
    # (b) cell 2 n + 1 takes the successor of cell 0 n + 4: its own successor is left without a predecessor
    sig_b = [row[:] for row in base.sig]
    orphan = cell_of[sig_b[2][1]]
    sig_b[2][1] = sig_b[0][4]
    assert orphan != cell_of[sig_b[0][4]]
    for sigma, needle in ((sig, "cell %d: not k_a w^b" % (n + 5)), (sig_b, "cell %d is the successor of no cell" % orphan)):
        inst = with_sigma(sigma)
        native = inst.native
        before = _outcome(mj, inst, wires)
        # without a table: none afterwards
        hb = native.hbm_bytes()
        assert L.mzk_prover_derive_wire_variables(native.handle, None) == INVALID and needle in L.mzk_last_error().decode(), L.mzk_last_error().decode()
        assert L.mzk_prover_get_wire_variables(native.handle, None, 0, C.byref(C.c_uint64())) == INVALID and native.hbm_bytes() == hb
        assert not native.check_witness(wires, base.pub).copy_checked
        # with a table: the same one afterwards
        mine = np.array(wv, dtype=np.uint32)[::-1].copy()
        native.set_wire_variables(mine, n_vars)
        nv = C.c_uint64(5)
        assert L.mzk_prover_derive_wire_variables(native.handle, C.byref(nv)) == INVALID and needle in L.mzk_last_error().decode()
        got, got_n = native.wire_variables()
        assert got_n == n_vars and np.array_equal(got, mine)
        assert _outcome(mj, inst, wires) == before
        native.release()
    # get: no table, short capacity, n_vars alone; unknown handles
    native = base.native
    out = np.zeros(W * n, dtype=np.uint32)
    nv = C.c_uint64()
    p = C.c_void_p(out.ctypes.data)
    assert L.mzk_prover_get_wire_variables(native.handle, p, W * n, C.byref(nv)) == INVALID
    assert L.mzk_prover_derive_wire_variables(native.handle, C.byref(nv)) == 0 and nv.value == n_vars
    assert L.mzk_prover_get_wire_variables(native.handle, p, W * n - 1, C.byref(nv)) == INVALID and not out.any()
    nv = C.c_uint64()
    assert L.mzk_prover_get_wire_variables(native.handle, None, 0, C.byref(nv)) == 0 and nv.value == n_vars
    assert L.mzk_prover_get_wire_variables(native.handle, p, W * n, None) == 0 and np.array_equal(out.reshape(W, n), np.array(wv, dtype=np.uint32))
    assert L.mzk_prover_derive_wire_variables(native.handle + 99, C.byref(nv)) == BAD_HANDLE
    assert L.mzk_prover_get_wire_variables(native.handle + 99, p, W * n, C.byref(nv)) == BAD_HANDLE
    assert _prove(mj, base, wires) == want
    base.release()
