// prover_round1.inc -- rounds 1 and 1.5 (prover.rs:72-118; constraint_system.rs:1225-1259, 1263-1417): wire / public-input polynomials, Plookup sorted vector.
// Member functions of ProverT (declared in prover.hip, which includes this file inside namespace mzk { namespace { ): one body per round
// of the reference's prover, as plonk/src/proof_system/prover.rs:72-419 has them.  No kernels here: every call is an entry point of the
// library (mzk_*_dev) on the handle's stream S.

template <class FrP, int CURVE>
void ProverT<FrP, CURVE>::public_input_row(const uint64_t* pi_rows, const uint64_t* pi, uint64_t n_pi) {
    void* d = coeff.at((size_t)W * n);
    ck(mzk_dev_memset(d, 0, n * EL, S));
    st.pi_zero = true;
    for (uint64_t i = 0; i < n_pi * 4 && st.pi_zero; i++) st.pi_zero = pi[i] == 0;
    if (st.pi_zero) return;
    if (n_pi > n) fail(MZK_ERR_INVALID_ARG, "more public inputs than rows");
    // staged through page-locked memory: asynchronous on the null stream, the caller's buffer is free when the call returns
    uint64_t* h = static_cast<uint64_t*>(stage_pi.reserve(n_pi * EL));
    std::memcpy(h, pi, n_pi * EL);
    if (!pi_rows) {
        ck(mzk_dev_upload_async(d, h, n_pi * EL, S));
    } else {
        for (uint64_t i = 0; i < n_pi; i++) {
            if (pi_rows[i] >= n) fail(MZK_ERR_INVALID_ARG, "public-input row outside the domain");
            ck(mzk_dev_upload_async(static_cast<uint8_t*>(d) + pi_rows[i] * EL, h + 4 * i, EL, S));
        }
    }
    ck(mzk_ntt_dev(CURVE, d, n, log_n, 1, nullptr, 1, n, S));      // compute_pub_input_polynomial (:1249-1259)
}

template <class FrP, int CURVE>
void ProverT<FrP, CURVE>::round1(int kind, const void* witness, uint64_t witness_len, const uint64_t* pi_rows, const uint64_t* pi, uint64_t n_pi,
        const uint64_t* blinders, uint64_t* out) {
    Tick tick(*this);
    st = State();
    stage = CREATED;
    timings_ms.clear();
    if (!witness || !blinders || !out || (n_pi && !pi)) fail(MZK_ERR_INVALID_ARG, "null pointer");
    if (S) ck(mzk_stream_wait_stream(S, nullptr));                 // what the caller wrote on the null stream (a device-resident witness) is complete first
    public_input_row(pi_rows, pi, n_pi);
    const size_t cells = (size_t)W * n;
    if (kind == MZK_WITNESS_DEV_WIRES) {
        if (witness_len != cells) fail(MZK_ERR_INVALID_ARG, "witness_len != num_wire_types * domain size");
        st.wire_values = witness;
        ck(mzk_dev_copy(coeff.p, witness, cells * EL, S));
        ck(mzk_ntt_dev(CURVE, coeff.p, n, log_n, 1, nullptr, W, n, S));
    } else if (kind == MZK_WITNESS_HOST_VECTOR || kind == MZK_WITNESS_DEV_VECTOR) {
        // the witness vector crosses PCIe; `witness[wire_variable(i, j)]` (constraint_system.rs:1239) is gathered on the device
        if (!vars_dev()) fail(MZK_ERR_STATE, "mzk_prover_set_wire_variables has not been called");
        if (witness_len != vars_n()) fail(MZK_ERR_INVALID_ARG, "witness_len != the n_vars of mzk_prover_set_wire_variables");
        if (!wv.p) wv.alloc(cells);
        st.wire_values = wv.p;
        const void* d_wit = witness;
        if (kind == MZK_WITNESS_HOST_VECTOR) {
            if (wit.elems < vars_n()) wit.alloc(vars_n());
            if (!copy_stream) ck(mzk_stream_create(&copy_stream));
            ck(mzk_stream_wait_stream(copy_stream, S));                                       // the previous proof is done with `wit`
            ck(mzk_dev_upload_async(wit.p, witness, vars_n() * EL, copy_stream));
            ck(mzk_stream_wait_stream(S, copy_stream));
            d_wit = wit.p;
        }
        ck(mzk_plonk_gather_witness_dev(d_wit, vars_n(), vars_dev(), cells, wv.p, S));
        ck(mzk_dev_copy(coeff.p, wv.p, cells * EL, S));
        ck(mzk_ntt_dev(CURVE, coeff.p, n, log_n, 1, nullptr, W, n, S));
    } else if (kind == MZK_WITNESS_HOST_WIRES) {
        // host-resident witness (constraint_system.rs:1225-1247 gathers it on the host): column i + 1 crosses PCIe on a copy
        // stream while column i is transformed on the null stream
        if (witness_len != cells) fail(MZK_ERR_INVALID_ARG, "witness_len != num_wire_types * domain size");
        if (!wv.p) wv.alloc(cells);
        if (!copy_stream) ck(mzk_stream_create(&copy_stream));
        st.wire_values = wv.p;
        ck(mzk_stream_wait_stream(copy_stream, S));                                           // the previous proof is done with `wv`
        for (int i = 0; i < W; i++) {
            ck(mzk_dev_upload_async(wv.at((size_t)i * n), static_cast<const uint8_t*>(witness) + (size_t)i * n * EL, n * EL, copy_stream));
            ck(mzk_stream_wait_stream(S, copy_stream));                                       // columns 0..i have arrived
            ck(mzk_dev_copy(coeff.at((size_t)i * n), wv.at((size_t)i * n), n * EL, S));
            ck(mzk_ntt_dev(CURVE, coeff.at((size_t)i * n), n, log_n, 1, nullptr, 1, n, S));
        }
    } else {
        fail(MZK_ERR_INVALID_ARG, "unknown witness_kind");
    }
    ck(mzk_dev_memset2d(static_cast<uint8_t*>(row(0)) + n * EL, (n + 3) * EL, 0, 3 * EL, (uint64_t)rows, S));   // the three tail slots of every row of the slab, one launch
    ck(mzk_dev_copy2d(slab.p, (n + 3) * EL, coeff.p, n * EL, n * EL, W, S));
    ck(mzk_dev_copy(row(rowPI()), coeff.at((size_t)W * n), n * EL, S));
    { std::vector<int> rs; for (int i = 0; i < W; i++) rs.push_back(i); mask(rs, blinders, 2); }
    tick.mark("r1_ntt_mask");
    std::vector<const void*> p; std::vector<uint64_t> l;
    if (key().srs_lagrange) {
        // sum_i v_i [L_i(beta)]g + b_0 [Z_H(beta)]g + b_1 [beta Z_H(beta)]g: rows of n + 3 slots, the values, then the blinders
        if (!vals_ext.p) vals_ext.alloc((size_t)W * (n + 3));
        ck(mzk_dev_copy2d(vals_ext.p, (n + 3) * EL, st.wire_values, n * EL, n * EL, W, S));
        for (int i = 0; i < W; i++)
            for (int j = 0; j < 2; j++) put_scalar(load(blinders + (size_t)(2 * i + j) * 4), vals_ext.at((size_t)i * (n + 3) + n + j));
        for (int i = 0; i < W; i++) { p.push_back(vals_ext.at((size_t)i * (n + 3))); l.push_back(n + 2); }
    } else {
        for (int i = 0; i < W; i++) { p.push_back(row(i)); l.push_back(n + 2); }
    }
    commit(p, l, out, key().srs_lagrange);                                // (synchronises the null stream, which has waited for the copy stream: the
    tick.mark("r1_commit");                                         // caller's host buffers are free again when this returns)
    stage = R1;
}

template <class FrP, int CURVE>
void ProverT<FrP, CURVE>::round1_5(const uint64_t* tau, const uint64_t* blinders, uint64_t* out) {
    if (!ultra) fail(MZK_ERR_UNSUPPORTED, "round 1.5 exists for UltraPlonk only");
    need(R1, R1_5, "round 1.5 follows round 1");
    Tick tick(*this);
    st.tau = load(tau);
    const int H1 = rowH1();
    ck(mzk_plookup_sorted_vec_dev(key().pk, st.wire_values, st.tau.l, table.p, lookup.p, sorted.p, S));
    ck(mzk_dev_copy(hh.p, sorted.p, n * EL, S));
    ck(mzk_dev_copy(hh.at(n), sorted.at(n - 1), n * EL, S));
    if (key().srs_lagrange) {
        // h_1, h_2 are committed from the sorted vector's VALUES (table entries and looked-up values: small numbers unless the circuit
        // looks up keyed tables) plus their three blinders, over the Lagrange-basis key -- as the wires in round 1
        if (!vals_ext.p) vals_ext.alloc((size_t)W * (n + 3));
        ck(mzk_dev_copy2d(vals_ext.p, (n + 3) * EL, hh.p, n * EL, n * EL, 2, S));
        for (int i = 0; i < 2; i++)
            for (int j = 0; j < 3; j++) put_scalar(load(blinders + (size_t)(3 * i + j) * 4), vals_ext.at((size_t)i * (n + 3) + n + j));
    }
    ck(mzk_ntt_dev(CURVE, hh.p, n, log_n, 1, nullptr, 2, n, S));
    ck(mzk_dev_copy2d(row(H1), (n + 3) * EL, hh.p, n * EL, n * EL, 2, S));
    mask({H1, H1 + 1}, blinders, 3);
    tick.mark("r1_5_sorted_vec");
    if (key().srs_lagrange) commit({vals_ext.p, vals_ext.at(n + 3)}, {n + 3, n + 3}, out, key().srs_lagrange);
    else commit({row(H1), row(H1 + 1)}, {n + 3, n + 3}, out);
    tick.mark("r1_5_commit");
    stage = R1_5;
}
