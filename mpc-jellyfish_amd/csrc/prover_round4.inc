// prover_round4.inc -- round 4 (prover.rs:216-299): evaluations at zeta and zeta * omega.
// Member functions of ProverT (declared in prover.hip, which includes this file inside namespace mzk { namespace { ): one body per round
// of the reference's prover, as plonk/src/proof_system/prover.rs:72-419 has them.  No kernels here: every call is an entry point of the
// library (mzk_*_dev) on the handle's stream S.

template <class FrP, int CURVE>
void ProverT<FrP, CURVE>::round4(const uint64_t* zeta_p, uint64_t* out_evals) {
    need(R3, R4, "round 4 follows round 3");
    Tick tick(*this);
    const Fr zeta = st.zeta = load(zeta_p);
    const Fr zeta_w = zeta * key().w_n;
    const int sigma0 = nsel, tab0 = nsel + W, H1 = rowH1(), PL = rowPL();
    EvalBatch ev(*this);
    // the wires and, in the same launch, z and the public-input polynomial (rows W, W + 1; every row is zero above its own length):
    // pi(zeta) is not part of the proof, the identity check of round 5 needs it
    const size_t h_w = ev.add(row(0), n + 3, W + 2, n + 3, zeta);
    const size_t h_s = ev.add(fix(sigma0), n, W - 1, n, zeta);
    const size_t h_z = ev.add(row(rowZ()), n + 3, 1, n + 3, zeta_w);
    size_t h_tz = 0, h_tn = 0, h_h1 = 0, h_ql = 0, h_qln = 0, h_pl = 0, h_hn = 0, h_wn = 0;
    if (ultra) {
        h_tz = ev.add(fix(tab0), n, 4, n, zeta);                                                           // range, key, table_dom_sep, q_dom_sep
        h_tn = ev.add(fix(tab0), n, 3, n, zeta_w);
        h_h1 = ev.add(row(H1), n + 3, 1, n + 3, zeta);
        h_ql = ev.add(fix(13), n, 1, n, zeta);
        h_qln = ev.add(fix(13), n, 1, n, zeta_w);
        h_pl = ev.add(row(PL), n + 3, 1, n + 3, zeta_w);
        h_hn = ev.add(row(H1), n + 3, 2, n + 3, zeta_w);
        h_wn = ev.add(row(3), n + 2, 2, n + 3, zeta_w);
    }
    ev.finish();
    const std::vector<Fr>& v = ev.vals;
    st.wires_evals.assign(v.begin() + h_w, v.begin() + h_w + W);
    st.pi_eval = v[h_w + W + 1];
    st.wire_sigma_evals.assign(v.begin() + h_s, v.begin() + h_s + W - 1);
    st.perm_next_eval = v[h_z];
    std::vector<Fr>& pe = st.plookup_evals;
    pe.clear();
    if (ultra) {
        pe.assign(N_PLOOKUP_EVALS, Fr::zero());
        pe[RANGE_TABLE] = v[h_tz]; pe[KEY_TABLE] = v[h_tz + 1]; pe[TABLE_DOM_SEP] = v[h_tz + 2]; pe[Q_DOM_SEP] = v[h_tz + 3];
        pe[RANGE_TABLE_NEXT] = v[h_tn]; pe[KEY_TABLE_NEXT] = v[h_tn + 1]; pe[TABLE_DOM_SEP_NEXT] = v[h_tn + 2];
        pe[H_1] = v[h_h1];
        pe[Q_LOOKUP] = v[h_ql];
        pe[Q_LOOKUP_NEXT] = v[h_qln];
        pe[PROD_NEXT] = v[h_pl];
        pe[H_1_NEXT] = v[h_hn]; pe[H_2_NEXT] = v[h_hn + 1];
        pe[W_3_NEXT] = v[h_wn]; pe[W_4_NEXT] = v[h_wn + 1];
    }
    uint64_t* o = out_evals;
    auto put = [&](const Fr& x) { std::memcpy(o, x.l, EL); o += 4; };
    for (auto& x : st.wires_evals) put(x);
    for (auto& x : st.wire_sigma_evals) put(x);
    put(st.perm_next_eval);
    for (auto& x : pe) put(x);
    tick.mark("r4_evals");
    stage = R4;
}
