// prover_round2.inc -- rounds 2 and 2.5 (prover.rs:125-183): permutation and Plookup grand products.
// Member functions of ProverT (declared in prover.hip, which includes this file inside namespace mzk { namespace { ): one body per round
// of the reference's prover, as plonk/src/proof_system/prover.rs:72-419 has them.  No kernels here: every call is an entry point of the
// library (mzk_*_dev) on the handle's stream S.

template <class FrP, int CURVE>
void ProverT<FrP, CURVE>::round2(const uint64_t* beta, const uint64_t* gamma, const uint64_t* blinders, uint64_t* out) {
    need(ultra ? R1_5 : R1, R2, ultra ? "round 2 follows round 1.5" : "round 2 follows round 1");
    Tick tick(*this);
    st.beta = load(beta); st.gamma = load(gamma);
    ck(mzk_plonk_perm_product_dev(key().pk, st.wire_values, st.beta.l, st.gamma.l, coeff.p, S));
    ck(mzk_dev_copy(row(rowZ()), coeff.p, n * EL, S));
    mask({rowZ()}, blinders, 3);
    tick.mark("r2_product");
    commit({row(rowZ())}, {n + 3}, out);
    tick.mark("r2_commit");
    stage = R2;
}

template <class FrP, int CURVE>
void ProverT<FrP, CURVE>::round2_5(const uint64_t* blinders, uint64_t* out) {
    if (!ultra) fail(MZK_ERR_UNSUPPORTED, "round 2.5 exists for UltraPlonk only");
    need(R2, R2_5, "round 2.5 follows round 2");
    Tick tick(*this);
    ck(mzk_plookup_product_dev(key().pk, table.p, lookup.p, sorted.p, st.beta.l, st.gamma.l, coeff.p, S));
    ck(mzk_dev_copy(row(rowPL()), coeff.p, n * EL, S));
    mask({rowPL()}, blinders, 3);
    tick.mark("r2_5_product");
    commit({row(rowPL())}, {n + 3}, out);
    tick.mark("r2_5_commit");
    stage = R2_5;
}
