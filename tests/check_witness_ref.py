"""The three definitions mzk_prover_check_witness is held to (include/mzk.h), on Python integers -- TEST INFRASTRUCTURE ONLY.

    gate     row i fails iff  pi + q_c + q_lc.w + q_mul0 w0 w1 + q_mul1 w2 w3 + q_hash.w^5 + q_ecc w0 w1 w2 w3 w4 - q_o w4 != 0
    lookup   row i < n - 1 passes iff some row j has (range[j], q tds[j], q key[j], q w3[j], q w4[j])
             = (w5[i], q' qds[i], q' w0[i], q' w1[i], q' w2[i]), q = q_lookup[j], q' = q_lookup[i]
    copy     the representative of a variable is its cell of smallest index wire * n + row; a cell fails iff its value differs

All arguments are lists of canonical integers as oracle/pyref_circuit.py builds them (selectors nsel x n, wires W x n, pi n values,
tables {"range", "key", "table_dom_sep", "q_dom_sep"} -> n values)."""


def gate_residual(c, sel, w, pi, i):
    r = c.r
    v = sum(sel[j][i] * w[j][i] for j in range(4)) + sel[4][i] * w[0][i] * w[1][i] + sel[5][i] * w[2][i] * w[3][i]
    v += sum(sel[6 + j][i] * pow(w[j][i], 5, r) for j in range(4))
    v += sel[12][i] * w[0][i] * w[1][i] * w[2][i] * w[3][i] * w[4][i] + sel[11][i] + pi[i] - sel[10][i] * w[4][i]
    return v % r


def gate_failures(c, sel, w, pi):
    """[(row, residual)] of the rows that fail the gate identity, in row order"""
    out = []
    for i in range(len(pi)):
        v = gate_residual(c, sel, w, pi, i)
        if v:
            out.append((i, v))
    return out


def lookup_failures(c, sel, w, tables):
    """rows i < n - 1 whose lookup tuple is carried by no table row, in row order"""
    r, n = c.r, len(w[0])
    q = sel[13]
    have = {(tables["range"][j] % r, q[j] * tables["table_dom_sep"][j] % r, q[j] * tables["key"][j] % r, q[j] * w[3][j] % r, q[j] * w[4][j] % r)
            for j in range(n)}
    return [i for i in range(n - 1)
            if (w[5][i] % r, q[i] * tables["q_dom_sep"][i] % r, q[i] * w[0][i] % r, q[i] * w[1][i] % r, q[i] * w[2][i] % r) not in have]


def copy_failures(w, wire_vars):
    """[(cell, representative cell)] of the cells whose value differs from their variable's first cell; cells as wire * n + row"""
    n = len(w[0])
    rep = {}
    for i, col in enumerate(wire_vars):
        for j, v in enumerate(col):
            rep.setdefault(v, i * n + j)
    out = []
    for i, col in enumerate(wire_vars):
        for j, v in enumerate(col):
            a = rep[v]
            if w[i][j] != w[a // n][a % n]:
                out.append((i * n + j, a))
    return out


def wire_variables_from_sigma(c, sigma, k, log_n):
    """A wire-variable table (W x n, number of variables) under which the copy constraints are those of sigma: cells in one sigma-cycle
    share a variable.  sigma[i][j] = k_a w^b names the cell (a, b) that follows (i, j); cells are found by inverting k_a w^b -> (a, b)."""
    n, r, W = 1 << log_n, c.r, len(sigma)
    w_n = c.root_of_unity(log_n)
    cell_of = {}
    for a in range(W):
        x = k[a] % r
        for b in range(n):
            cell_of[x] = (a, b)
            x = x * w_n % r
    var = [[None] * n for _ in range(W)]
    n_vars = 0
    for i in range(W):
        for j in range(n):
            if var[i][j] is not None:
                continue
            a, b = i, j
            while var[a][b] is None:
                var[a][b] = n_vars
                a, b = cell_of[sigma[a][b]]
            n_vars += 1
    return var, n_vars


def expected_report(c, sel, w, pi, tables=None, wire_vars=None):
    """what the report must hold for this witness: {"kind", "gate": [(row, residual)], "lookup": [rows], "copy": [(cell, rep)] | None}"""
    gate = gate_failures(c, sel, w, pi)
    lookup = lookup_failures(c, sel, w, tables) if tables is not None else []
    copy = copy_failures(w, wire_vars) if wire_vars is not None else None
    kind = "gate" if gate else "lookup" if lookup else "copy" if copy else "satisfied"
    return {"kind": kind, "gate": gate, "lookup": lookup, "copy": copy}
