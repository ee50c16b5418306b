// prover_round5.inc -- round 5 (prover.rs:302-460, 490-509, 963-1112): linearisation polynomial, batched opening proofs, the quotient identity at zeta.
// Member functions of ProverT (declared in prover.hip, which includes this file inside namespace mzk { namespace { ): one body per round
// of the reference's prover, as plonk/src/proof_system/prover.rs:72-419 has them.  No kernels here: every call is an entry point of the
// library (mzk_*_dev) on the handle's stream S.

// compute_non_quotient_component_for_lin_poly (prover.rs:302-337, 963-1112) as terms, every scalar times alpha_base
template <class FrP, int CURVE>
auto ProverT<FrP, CURVE>::lin_poly_terms(const Fr& alpha_base) const -> std::vector<Term> {
    const std::vector<Fr>& we = st.wires_evals;
    const std::vector<Fr>& pe = st.plookup_evals;
    const Fr &alpha = st.alpha, &beta = st.beta, &gamma = st.gamma, &tau = st.tau, &zeta = st.zeta;
    const int sigma0 = nsel;
    auto pow5 = [](const Fr& x) { const Fr x2 = x * x; return x2 * x2 * x; };
    std::vector<Term> terms;
    for (int j = 0; j < 4; j++) terms.push_back({we[j], fix(j), n});
    terms.push_back({we[0] * we[1], fix(4), n});
    terms.push_back({we[2] * we[3], fix(5), n});
    for (int j = 0; j < 4; j++) terms.push_back({pow5(we[j]), fix(6 + j), n});
    terms.push_back({we[0] * we[1] * we[2] * we[3] * we[4], fix(12), n});
    terms.push_back({neg(we[4]), fix(10), n});
    terms.push_back({Fr::one(), fix(11), n});
    const Fr one = Fr::one(), nf = from_u64<FrP>(n);
    const Fr vanish = pow_u64(zeta, n) - one;
    const Fr lagrange_1 = vanish * inv(nf * (zeta - one));
    Fr cf = alpha;
    for (int j = 0; j < W; j++) cf = cf * (we[j] + beta * key().k[j] * zeta + gamma);
    terms.push_back({cf + alpha * alpha * lagrange_1, row(rowZ()), n + 3});
    cf = alpha * beta * st.perm_next_eval;
    for (int j = 0; j < W - 1; j++) cf = cf * (we[j] + beta * st.wire_sigma_evals[j] + gamma);
    terms.push_back({neg(cf), fix(sigma0 + W - 1), n});
    if (ultra) {                                                                                          // compute_lin_poly_plookup_contribution
        auto em = [&](const Fr& first, const Fr& ql, const Fr& ds, const Fr& a0, const Fr& a1, const Fr& a2) {
            return first + ql * tau * (ds + tau * (a0 + tau * (a1 + tau * a2)));
        };
        const Fr mt = em(pe[RANGE_TABLE], pe[Q_LOOKUP], pe[TABLE_DOM_SEP], pe[KEY_TABLE], we[3], we[4]);
        const Fr mt_next = em(pe[RANGE_TABLE_NEXT], pe[Q_LOOKUP_NEXT], pe[TABLE_DOM_SEP_NEXT], pe[KEY_TABLE_NEXT], pe[W_3_NEXT], pe[W_4_NEXT]);
        const Fr ml = em(we[5], pe[Q_LOOKUP], pe[Q_DOM_SEP], we[0], we[1], we[2]);
        const Fr w_inv = inv(key().w_n);
        const Fr lagrange_n = vanish * w_inv * inv(nf * (zeta - w_inv));
        const Fr a2 = alpha * alpha, a4 = a2 * a2, a5 = a4 * alpha, a6 = a4 * a2;
        const Fr b1 = one + beta, g1 = gamma * b1, zmg = zeta - w_inv;
        terms.push_back({a4 * lagrange_1 + a5 * lagrange_n + a6 * zmg * b1 * (gamma + ml) * (g1 + mt + beta * mt_next), row(rowPL()), n + 3});
        terms.push_back({neg(a6 * zmg * pe[PROD_NEXT] * (g1 + pe[H_1] + beta * pe[H_1_NEXT])), row(rowH1() + 1), n + 3});
    }
    if (!(alpha_base == one)) for (auto& t : terms) t.s = t.s * alpha_base;
    return terms;
}

// What the verifier takes for -(linearisation polynomial)(zeta): Verifier::compute_lin_poly_constant_term (verifier.rs:340-414) for this
// instance, times alpha_base.  The prover knows every input: its own evaluations and pi(zeta).
template <class FrP, int CURVE>
auto ProverT<FrP, CURVE>::lin_poly_constant(const Fr& alpha_base) const -> Fr {
    const std::vector<Fr>& we = st.wires_evals;
    const std::vector<Fr>& pe = st.plookup_evals;
    const Fr &alpha = st.alpha, &beta = st.beta, &gamma = st.gamma, &zeta = st.zeta;
    const Fr one = Fr::one(), nf = from_u64<FrP>(n), a2 = alpha * alpha;
    const Fr vanish = pow_u64(zeta, n) - one;
    const Fr lagrange_1 = vanish * inv(nf * (zeta - one));
    Fr t = st.pi_eval - a2 * lagrange_1;
    Fr acc = alpha * st.perm_next_eval * (gamma + we[W - 1]);
    for (int j = 0; j < W - 1; j++) acc = acc * (gamma + we[j] + beta * st.wire_sigma_evals[j]);
    t = t - acc;
    if (ultra) {
        const Fr a3 = a2 * alpha, w_inv = inv(key().w_n);
        const Fr lagrange_n = vanish * w_inv * inv(nf * (zeta - w_inv));
        const Fr g1 = gamma * (one + beta);
        const Fr pc = lagrange_n * (pe[H_1] - pe[H_2_NEXT] - a2) - alpha * lagrange_1
                      - a3 * (zeta - w_inv) * pe[PROD_NEXT] * (g1 + pe[H_1] + beta * pe[H_1_NEXT]) * (g1 + beta * pe[H_2_NEXT]);
        t = t + a3 * pc;
    }
    return t * alpha_base;
}

// the evaluations at zeta in the order of open_lists' first list (after the linearisation polynomial)
template <class FrP, int CURVE>
void ProverT<FrP, CURVE>::opened_evals(std::vector<Fr>& out) const {
    out.insert(out.end(), st.wires_evals.begin(), st.wires_evals.end());
    out.insert(out.end(), st.wire_sigma_evals.begin(), st.wire_sigma_evals.end());
    if (ultra) {
        const std::vector<Fr>& pe = st.plookup_evals;
        for (int i : {RANGE_TABLE, KEY_TABLE, H_1, Q_LOOKUP, TABLE_DOM_SEP, Q_DOM_SEP}) out.push_back(pe[i]);
    }
}

// compute_quotient_component_for_lin_poly (prover.rs:343-358) over this->split
template <class FrP, int CURVE>
auto ProverT<FrP, CURVE>::quotient_lin_terms(const Fr& zeta) const -> std::vector<Term> {
    const Fr one = Fr::one(), vanish = pow_u64(zeta, n) - one, zeta_n2 = (vanish + one) * zeta * zeta;
    std::vector<Term> terms;
    Fr cf = one;
    for (int i = 0; i < W; i++) {
        terms.push_back({neg(vanish) * cf, split.at((size_t)i * (n + 3)), st.split_len[i]});
        cf = cf * zeta_n2;
    }
    return terms;
}

// the polynomials this instance opens at zeta (after the linearisation polynomial) and at zeta * w (prover.rs:362-460)
template <class FrP, int CURVE>
void ProverT<FrP, CURVE>::open_lists(std::vector<Term>& open_polys, std::vector<Term>& shifted_polys) const {
    const Fr one = Fr::one();
    const int sigma0 = nsel, tab0 = nsel + W, H1 = rowH1(), PL = rowPL();
    for (int i = 0; i < W; i++) open_polys.push_back({one, row(i), n + 2});
    for (int i = 0; i < W - 1; i++) open_polys.push_back({one, fix(sigma0 + i), n});
    shifted_polys.push_back({one, row(rowZ()), n + 3});
    if (ultra) {
        for (const void* p : {(const void*)fix(tab0), (const void*)fix(tab0 + 1)}) open_polys.push_back({one, p, n});
        open_polys.push_back({one, row(H1), n + 3});
        open_polys.push_back({one, fix(13), n});
        open_polys.push_back({one, fix(tab0 + 2), n});
        open_polys.push_back({one, fix(tab0 + 3), n});
        shifted_polys.push_back({one, row(PL), n + 3});
        shifted_polys.push_back({one, fix(tab0), n});
        shifted_polys.push_back({one, fix(tab0 + 1), n});
        shifted_polys.push_back({one, row(H1), n + 3});
        shifted_polys.push_back({one, row(H1 + 1), n + 3});
        shifted_polys.push_back({one, fix(13), n});
        shifted_polys.push_back({one, row(3), n + 2});
        shifted_polys.push_back({one, row(4), n + 2});
        shifted_polys.push_back({one, fix(tab0 + 2), n});
    }
}

// compute_batched_witness_polynomial_commitment (prover.rs:490-509) up to the commitment
template <class FrP, int CURVE>
void ProverT<FrP, CURVE>::batched_witness(const std::vector<Term>& polys, const Fr& v, const Fr& point, Buf& out, void* d_rem) {
    std::vector<Term> t;
    Fr c = Fr::one();
    for (auto& p : polys) { t.push_back({c, p.p, p.len}); c = c * v; }
    lincomb_many(t, batch.p, n + 3);
    if (d_rem) ck(mzk_poly_div_linear_rem_dev(CURVE, batch.p, n + 3, point.l, out.p, d_rem, S));   // remainder = batch(point)
    else ck(mzk_poly_div_linear_dev(CURVE, batch.p, n + 3, point.l, out.p, S));
}

// Round 5 over several ranks (SURVEY.md 8(e)).  The opening witness of a batch polynomial b at a point z is
// w_j = sum_{i > j} b_i z^(i-j-1).  A rank needs w on its own coefficient range [lo, hi) only -- that is its MSM shard -- and
// w_j = (the same sum over i < hi) + z^(hi-1-j) S_hi with S_hi = sum_{i >= hi} b_i z^(i-hi): the higher ranks' contribution enters
// as ONE field element.  So: linear combinations on the range only (they are pointwise); e = the range read as a polynomial,
// evaluated at z; one all-gather of the e's; S_hi appended as an extra top coefficient, after which the ordinary division by
// (X - z) of the extended range returns exactly w on the range; commit over the range.
template <class FrP, int CURVE>
void ProverT<FrP, CURVE>::openings_ranged(const std::vector<Term>& lin_terms, const std::vector<Term>& open_polys,
        const std::vector<Term>& shifted_polys, const Fr& v, const Fr& zeta, Tick& tick, uint64_t* out) {
    const uint64_t hi_c = std::min<uint64_t>(hi, n + 3), width = hi_c > lo ? hi_c - lo : 0;
    auto cut = [&](const std::vector<Term>& terms) {
        std::vector<Term> o;
        for (auto& t : terms) {
            const uint64_t a = std::min(lo, t.len), b = std::min(hi_c, t.len);
            if (b > a) o.push_back({t.s, static_cast<const uint8_t*>(t.p) + a * EL, b - a});
        }
        return o;
    };
    const Fr zw = zeta * key().w_n;
    std::vector<Term> open_terms = lin_terms, shift_terms;         // 1 * lin + sum_i v^(i+1) p_i
    Fr c = v;
    for (auto& p : open_polys) { open_terms.push_back({c, p.p, p.len}); c = c * v; }
    c = Fr::one();
    for (auto& p : shifted_polys) { shift_terms.push_back({c, p.p, p.len}); c = c * v; }
    // batch.p: the open batch's range, then ONE carried coefficient; lin.p: the same for the shifted batch
    void* bufs[2] = {batch.p, lin.p};
    const std::vector<Term> cuts[2] = {cut(open_terms), cut(shift_terms)};
    const Fr points[2] = {zeta, zw};
    Fr e[2] = {Fr::zero(), Fr::zero()};
    for (int j = 0; j < 2; j++) {
        if (!width) continue;
        if (cuts[j].empty()) ck(mzk_dev_memset(bufs[j], 0, width * EL, S));
        else lincomb_many(cuts[j], bufs[j], width);
        e[j] = evaluate(bufs[j], width, 1, width, points[j])[0];
    }
    std::vector<Fr> every((size_t)2 * world);
    if (comm.all_gather(comm.ctx, e, sizeof e, every.data())) fail(MZK_ERR_INVALID_ARG, "mzk_comm.all_gather failed");
    st.batch_at_zeta = Fr::zero();                                  // the open batch polynomial's value at zeta: every rank's range value times zeta^lo
    for (int q = 0; q < world; q++)
        st.batch_at_zeta = st.batch_at_zeta + pow_u64(zeta, std::min<uint64_t>(shard_range(n + 3, q, world).first, n + 3)) * every[2 * q];
    Fr carry[2] = {Fr::zero(), Fr::zero()};
    for (int q = rank + 1; q < world; q++) {                       // S_hi: the ranges above, shifted down to start at hi
        const uint64_t lo_q = std::min<uint64_t>(shard_range(n + 3, q, world).first, n + 3);
        for (int j = 0; j < 2; j++) carry[j] = carry[j] + pow_u64(points[j], lo_q - hi_c) * every[2 * q + j];
    }
    void* outs[2] = {opening.p, shifted.p};
    for (int j = 0; j < 2 && width; j++) {
        put_scalar(carry[j], static_cast<uint8_t*>(bufs[j]) + width * EL);                                    // the carried coefficient, without a copy
        ck(mzk_poly_div_linear_dev(CURVE, bufs[j], width + 1, points[j].l, outs[j], S));               // width coefficients: w on [lo, hi)
    }
    tick.mark("r5_polys");
    commit_slices({opening.p, shifted.p}, {width, width}, out);
    tick.mark("r5_commit");
}

template <class FrP, int CURVE>
void ProverT<FrP, CURVE>::round5(const std::vector<ProverBase*>& inst, const uint64_t* v_p, uint64_t* out) {
    Tick tick(*this);
    if (st.bases.size() != inst.size()) fail(MZK_ERR_STATE, "round 5 takes the instances of round 3, first instance first");
    for (ProverBase* b : inst) {
        static_cast<ProverT*>(b)->need(R4, R4 + 1, "round 5 follows round 4 of every instance");
        if (b != this) ck(mzk_stream_wait_stream(S, b->S));         // the other instances' polynomials are read on this stream
    }
    const Fr v = load(v_p), zeta = st.zeta;
    std::vector<Term> terms = quotient_lin_terms(zeta);
    for (size_t i = 0; i < inst.size(); i++) {
        ProverT* p = static_cast<ProverT*>(inst[i]);
        if (!(p->st.zeta == zeta)) fail(MZK_ERR_STATE, "round 4 of the instances used different evaluation challenges");
        const std::vector<Term> t = p->lin_poly_terms(st.bases[i]);
        terms.insert(terms.end(), t.begin(), t.end());
    }
    std::vector<Term> open_polys, shifted_polys;
    if (world > 1) {
        open_lists(open_polys, shifted_polys);
        openings_ranged(terms, open_polys, shifted_polys, v, zeta, tick, out);
    } else {
        lincomb_many(terms, lin.p, n + 3);
        open_polys.push_back({Fr::one(), lin.p, n + 3});
        for (ProverBase* b : inst) static_cast<ProverT*>(b)->open_lists(open_polys, shifted_polys);
        batched_witness(open_polys, v, zeta, opening, rem_dev());
        batched_witness(shifted_polys, v, zeta * key().w_n, shifted);
        ck(mzk_dev_download_async(static_cast<uint8_t*>(stage_back.reserve(64)) + 32, rem_dev(), EL, S));       // read after the commitments, copied before them
        tick.mark("r5_polys");
        commit({opening.p, shifted.p}, {n + 2, n + 2}, out);
        tick.mark("r5_commit");
        sync_stream();
        std::memcpy(st.batch_at_zeta.l, static_cast<const uint8_t*>(stage_back.p) + 32, EL);
    }
    for (ProverBase* b : inst) b->stage = CREATED;
    // t(X) Z_H(X) = numerator(X), checked at the evaluation challenge the way the verifier will check it (verifier.rs:186-231, 340-414):
    // the opening proof's batch polynomial lin + sum_i v^i p_i must take the value -r_0 + sum_i v^i p_i(zeta) at zeta, and its value there
    // is the remainder its division by (X - zeta) leaves: one 32-byte read.  The guard against an unsatisfied witness where the top
    // coefficients of the quotient come from its numerator -- reported under the reference's error name (prover.rs:915-918).
    Fr lin_constant = Fr::zero();
    std::vector<Fr> opened;
    for (size_t i = 0; i < inst.size(); i++) {
        ProverT* p = static_cast<ProverT*>(inst[i]);
        lin_constant = lin_constant + p->lin_poly_constant(st.bases[i]);
        p->opened_evals(opened);
    }
    Fr want = neg(lin_constant), c = Fr::one();
    for (auto& e : opened) { c = c * v; want = want + c * e; }
    if (!(st.batch_at_zeta == want))
        fail(MZK_ERR_WRONG_QUOTIENT_DEGREE, "WrongQuotientPolyDegree: the quotient identity t(X) Z_H(X) = numerator(X) does not hold at the evaluation "
                                            "challenge (the witness does not satisfy the circuit)");
}
