"""CPU: the integer restatement of the witness check's definitions (tests/check_witness_ref.py) agrees with the oracle's own row check
on satisfied and corrupted circuits, and the library exports the entry point with the report layout the ctypes client declares."""
import ctypes as C
import random
import re
import os

import pytest

import check_witness_ref as REF
import pyref_circuit as PC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("curve_id,log_n,gates", [(0, 3, "hot"), (1, 6, "hot"), (0, 6, "all"), (1, 9, "all")])
def test_reference_agrees_with_the_oracle_on_turbo_circuits(pyref, curve_id, log_n, gates):
    c = pyref.CURVES[curve_id]
    n = 1 << log_n
    rng = random.Random(8800 + curve_id + log_n)
    sel, sig, k, w, pi = PC.general_circuit(c, log_n, rng, gates=gates)
    assert PC.check_gate_rows(c, sel, w, pi)
    wv, n_vars = REF.wire_variables_from_sigma(c, sig, k, log_n)
    assert n_vars < 5 * n and all(0 <= v < n_vars for col in wv for v in col)
    assert REF.expected_report(c, sel, w, pi, None, wv) == {"kind": "satisfied", "gate": [], "lookup": [], "copy": []}
    # one changed output: the oracle's row check refuses the circuit, the reference names the row and its residual
    row = next(i for i in range(n) if sel[10][i])
    w[4][row] = (w[4][row] + 1) % c.r
    assert not PC.check_gate_rows(c, sel, w, pi)
    fails = REF.gate_failures(c, sel, w, pi)
    assert fails == [(row, -sel[10][row] % c.r)]
    # a public input the circuit does not hold fails on its row
    w[4][row] = (w[4][row] - 1) % c.r
    assert REF.gate_failures(c, sel, w, [0] * n) == [(3, 5)]
    # a changed cell of a 3-cycle: one failure when it is not the representative, two when it is
    cyc = next(cells for cells in _cycles(wv, n) if len(cells) == 3)
    for pos, want in ((1, [(cyc[1], cyc[0])]), (0, [(cyc[1], cyc[0]), (cyc[2], cyc[0])])):
        bad = [col[:] for col in w]
        bad[cyc[pos] // n][cyc[pos] % n] = (bad[cyc[pos] // n][cyc[pos] % n] + 1) % c.r
        assert REF.copy_failures(bad, wv) == want


def _cycles(wv, n):
    by = {}
    for i, col in enumerate(wv):
        for j, v in enumerate(col):
            by.setdefault(v, []).append(i * n + j)
    return by.values()


@pytest.mark.parametrize("curve_id,log_n,gates,range_bits", [(1, 4, "hot", 2), (0, 6, "hot", 3), (1, 6, "all", 3), (0, 8, "all", 3)])
def test_reference_on_ultra_circuits(pyref, curve_id, log_n, gates, range_bits):
    c = pyref.CURVES[curve_id]
    n, R = 1 << log_n, 1 << range_bits
    rng = random.Random(8900 + curve_id + log_n)
    sel, sig, k, w, pi, tabs = PC.general_ultra_circuit(c, log_n, rng, range_bits=range_bits, gates=gates)
    wv, _ = REF.wire_variables_from_sigma(c, sig, k, log_n)
    assert REF.expected_report(c, sel, w, pi, tabs, wv) == {"kind": "satisfied", "gate": [], "lookup": [], "copy": []}
    bad = [col[:] for col in w]
    bad[1][R + 1] = (bad[1][R + 1] + 1) % c.r                    # a looked-up value of lookup row R + 1
    assert REF.lookup_failures(c, sel, bad, tabs) == [R + 1] and not REF.gate_failures(c, sel, bad, pi)
    bad = [col[:] for col in w]
    bad[5][0] = R                                                # one past the range table
    assert REF.lookup_failures(c, sel, bad, tabs) == [0]
    bad = [col[:] for col in w]
    bad[5][n - 1] = c.r - 1                                      # the last row is not looked up
    assert REF.lookup_failures(c, sel, bad, tabs) == []


def test_reference_on_the_bench_circuit(pyref):
    c = pyref.CURVES[1]
    k = [1, 7, 13, 17, 23, 29]
    n, wires, witness, sel, sigma, tables = PC.bench_circuit(c, 40, True, 3, k)
    w = [[witness[v] for v in col] for col in wires]
    assert REF.expected_report(c, sel, w, [0] * n, tables, wires) == {"kind": "satisfied", "gate": [], "lookup": [], "copy": []}
    wv, n_vars = REF.wire_variables_from_sigma(c, sigma, k, n.bit_length() - 1)
    assert n_vars == len(witness) and REF.copy_failures(w, wv) == []


def test_library_exports_the_check_and_the_report_layout(mj):
    L = mj.load()
    assert hasattr(L, "mzk_prover_check_witness")
    from importlib import import_module
    lib = import_module("mpc-jellyfish_amd.lib")
    assert "mzk_prover_check_witness" in lib.EXPORTS
    # the ctypes structure follows the header's field list
    text = open(os.path.join(ROOT, "include", "mzk.h")).read()
    body = re.search(r"typedef struct mzk_witness_report \{(.*?)\} mzk_witness_report;", text, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    names = [re.sub(r"\[.*", "", x).strip() for decl in body.split(";") if decl.strip() for x in decl.split(None, 1)[1].split(",")]
    assert names == [f[0] for f in lib.WitnessReport._fields_]
    assert C.sizeof(lib.WitnessReport) == 8 + 7 * 8 + 24 * 8 + 4 * 8
    assert lib.WitnessReport.row_wires.offset == 64 and lib.WitnessReport.gate_residual.offset == 256
